"""Sub-graph proposals on the device (subgc.proposals, eval_glue.caption_scene_graphs) against the numpy restatements of their contracts
(tests/test_proposals_cpu.py works those by hand), the reference loader's own rows for the expansion step, and -- for the items and the
captions -- a second route through `assemble_test_batch` with the sampler's candidates fed back as precomputed ones.
Shapes: the golden tiny sGPN model, obj_num 37, rel_num 65, three images, 24 draws each from 1..3 seeds."""
import numpy as np
import pytest
import torch

import sct_loader_golden as G
from subgc import control_input as CI
from subgc import eval_glue, synthetic
from subgc import proposals as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_DRAW, SEEDS, SEED, OBJ, REL, D, N_CLS, N_PRED = 24, (1, 3), 2019, 37, 65, 64, 1599, 21
IDS = [1000, 1001, 1002]
ITEM_KEYS = ("fc_feats", "att_feats", "obj_dist", "rel_ind", "pred_dist", "gpn_obj_ind", "att_masks", "gpn_pool_mtx", "gpn_pred_ind", "gpn_nrel_ind")


def _image(seed, n_edges, two_classes=False, one_class=False):
    """One image's raw arrays on the host, from the synthetic generator's scene graph."""
    g = synthetic.make_graph(np.random.default_rng(seed), 1, OBJ, REL, D, N_CLS, N_PRED, n_edges=n_edges)
    dist, rel = g["obj_dist"][0, :OBJ - 1].copy(), g["rel_ind"][0, :n_edges].copy()
    if two_classes or one_class:                                  # nodes 0..17 of class 3, 18..35 of class 9 (or all of class 3); relations inside a class
        dist[:] = 0.01
        dist[:18, 3] = 0.9
        dist[18:, 3 if one_class else 9] = 0.9
        rel = np.array([[0, 1], [2, 3], [20, 21]], np.int64)[:n_edges]
    return dict(object_fmap=g["att_feats"][0, :OBJ - 1], object_dist=dist, rel_ind=rel, pred_dist=g["pred_dist"][0, :n_edges])


def _raw(images):
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dt)
    return dict(object_fmap=t(np.stack([im["object_fmap"] for im in images])), object_dist=t(np.stack([im["object_dist"] for im in images])),
                rel_ind=t(np.concatenate([im["rel_ind"] for im in images]).reshape(-1, 2), torch.int64),
                pred_dist=t(np.concatenate([im["pred_dist"] for im in images]).reshape(-1, N_PRED)),
                rel_off=t(np.cumsum([0] + [im["rel_ind"].shape[0] for im in images]), torch.int64))


@pytest.fixture(scope="module")
def images():
    return [_image(500, 20), _image(501, 0), _image(502, 3, two_classes=True)]     # the generator's; no relation at all; two classes only


@pytest.fixture(scope="module")
def sampler():
    return P.ProposalSampler(N_DRAW, SEEDS, SEED, OBJ, REL)


@pytest.fixture(scope="module")
def drawn(images, sampler):
    return sampler.sample(_raw(images), keys=IDS)


@pytest.fixture(scope="module")
def restated(images):
    """The whole chain in numpy, image by image: seeds -> expansion -> duplicate removal."""
    out = []
    for k, im in zip(IDS, images):
        seed, _, _, _ = P.restate_seeds(N_DRAW, OBJ - 1, SEEDS, SEED, k)
        rows = P.restate_extract(seed, im["object_dist"], im["rel_ind"], OBJ, REL)
        kept, used = P.restate_dedup(rows["node_mask"])
        out.append(dict(seed=seed, rows=rows, kept=kept, used=used))
    return out


@pytest.fixture(scope="module")
def model():
    import conftest
    import subgc.models as models
    g = conftest.Golden("subgc_greedy")
    w = conftest.Golden("subgc_beam").group("weights")
    w["logit.bias"][0] += 2.0
    m = models.setup(g.opt(caption_model="topdown", gpn_drop_prob=0.0, sct=0))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return m.to(DEV).eval()


VOCAB = {str(i): f"w{i}" for i in range(1, 60)}


# ---- 1. seeds ----------------------------------------------------------------------------------------------------------------------------

def test_seed_masks_from_injected_uniforms_equal_the_restatement(sampler):
    rng = np.random.default_rng(7)
    U = rng.random((3, N_DRAW, OBJ - 1), dtype=np.float32)
    w = rng.random((3, N_DRAW), dtype=np.float32)
    U[0, 0, 5] = U[0, 0, 30] = 2.0                    # two equal maxima: the lower column is the first seed
    U[0, 1, :] = 0.25                                 # every value equal: columns 0, 1, 2
    U[1, 2, 35] = U[1, 2, 0] = 3.0                    # a tie across the row's ends
    w[0, 0], w[0, 1], w[1, 2] = 0.0, 1.0, np.float32(1) - np.float32(2.0 ** -24)   # s = 1; the clamp (floor(3.0) = 3 -> 2); the largest stream value
    w[2, 0], w[2, 1] = np.float32(1 / 3), np.float32(2 / 3)                        # the fp32 product decides, not the real one
    seed, _, _ = sampler.draw_seeds(3, OBJ - 1, IDS, DEV, uniforms=(U, w))
    got = seed.cpu().numpy().view(np.uint64).reshape(3, N_DRAW)
    for b in range(3):
        want, s, _, _ = P.restate_seeds(N_DRAW, OBJ - 1, SEEDS, SEED, IDS[b], U=U[b], w=w[b])
        assert got[b].tolist() == want.tolist(), b
    assert int(got[0, 0]) == 1 << 5 and int(got[0, 1]) == 0b111 and int(got[1, 2]) == (1 << 0) | (1 << 35) | (1 << int(np.argsort(-U[1, 2], kind="stable")[2]))
    wide = P.ProposalSampler(4, (5, 32), SEED, OBJ, REL)                            # k > 4: the top-k kernel's other form
    U4, w4 = rng.random((1, 4, OBJ - 1), dtype=np.float32), np.array([[0.0, 0.5, 0.99, 1.0]], np.float32)
    got = wide.draw_seeds(1, OBJ - 1, [0], DEV, uniforms=(U4, w4))[0].cpu().numpy().view(np.uint64)
    want, s, _, _ = P.restate_seeds(4, OBJ - 1, (5, 32), SEED, 0, U=U4[0], w=w4[0])
    assert got.tolist() == want.tolist() and s.tolist() == [5, 19, 32, 32]


def test_the_devices_own_stream_equals_the_restated_one(sampler):
    """Without injection: U, w and the masks of keys far apart are the restated Philox values at the contract's offsets, bit for bit."""
    keys = [0, 1001, (1 << 43) - 1]
    seed, U, w = sampler.draw_seeds(3, OBJ - 1, keys, DEV)
    seed, U, w = seed.cpu().numpy().view(np.uint64).reshape(3, -1), U.cpu().numpy().reshape(3, N_DRAW, -1), w.cpu().numpy().reshape(3, -1)
    for b, k in enumerate(keys):
        want, _, rU, rw = P.restate_seeds(N_DRAW, OBJ - 1, SEEDS, SEED, k)
        assert U[b].tobytes() == rU.tobytes() and w[b].tobytes() == rw.tobytes() and seed[b].tolist() == want.tolist(), k


# ---- 2. extraction, pinned on the reference loader's rows ---------------------------------------------------------------------------------

@pytest.mark.parametrize("tags", [("g0", "g1", "g2", "g4"), ("g3",)])
def test_extract_equals_the_reference_loaders_rows(tags):
    meta, arr = G.load()
    info = meta["images"][tags[0]]
    raw, sets, off, wh, _ = G.raw_batch(meta, arr, tags, DEV, only_ok=True)
    d_off = torch.tensor(off, dtype=torch.int64, device=DEV)
    seed, _, _, status = CI.match_regions(raw["boxes"], torch.tensor(wh, dtype=torch.float32, device=DEV), sets, d_off)
    assert not status.cpu().any()
    s = P.ProposalSampler(2, (1, 1), 0, info["obj_num"], info["rel_num"])
    rows = s.extract(raw, seed, off)
    again = s.extract(raw, seed.cpu().numpy().view(np.uint64), off)                 # host masks as uint64: the same call
    for b, tag in enumerate(tags):
        want = G.expected(meta, arr, tag)
        assert (rows["object_cls"][b].cpu().numpy() == np.argmax(arr[f"{tag}_object_dist"], 1)).all(), tag
        for k in G.ROWS:
            got = rows[k][off[b]:off[b + 1]].cpu().numpy()
            w = want[k][0, 0]                                                      # the sct item shows one row per set in both halves
            assert got.shape == w.shape and got.dtype == w.dtype and got.tobytes() == np.ascontiguousarray(w).tobytes(), (tag, k)
            assert torch.equal(rows[k], again[k]), k


# ---- 3. duplicate removal -------------------------------------------------------------------------------------------------------------------

def test_kept_lists_equal_the_restatement(drawn, restated):
    t = drawn.table
    assert t["kept"].tolist() == [len(r["kept"]) for r in restated] and t["used"].tolist() == [r["used"] for r in restated]
    assert t["off"].tolist() == np.concatenate([[0], np.cumsum(t["kept"])]).tolist()
    for b, r in enumerate(restated):
        a, e = t["off"][b], t["off"][b + 1]
        draw = t["draw"][a:e]
        assert draw.tolist() == r["kept"].tolist(), b
        assert t["seed_mask"][a:e].tolist() == r["seed"][draw].tolist() and t["node_mask"][a:e].tolist() == r["rows"]["node_mask"][draw].tolist(), b
        assert len(set(t["node_mask"][a:e].tolist())) == e - a                                  # kept node sets are pairwise distinct
        every = r["rows"]["node_mask"]
        for j in sorted(set(range(N_DRAW)) - set(draw.tolist())):                                # a dropped candidate repeats an EARLIER kept one
            assert any(int(every[i]) == int(every[j]) for i in draw.tolist() if i < j), (b, j)
        assert drawn.items[b]["this_mini_batch"] == r["used"] // 2
    assert t["kept"][0] > 10                                                                     # the generator's image: mostly distinct
    # two classes: a candidate is one class, the other, or both -- nearly all of the 24 collapse, and an odd survivor is not used
    assert t["kept"][2] <= len(set(restated[2]["rows"]["node_mask"].tolist())) <= 3 and t["kept"][2] >= 2
    assert (t["kept"][2], t["used"][2]) == (3, 2)


def test_an_image_with_fewer_than_two_distinct_candidates_raises_naming_its_key(images, sampler):
    raw = _raw([images[0], _image(503, 3, one_class=True)])
    with pytest.raises(ValueError, match=r"image key 77 is left with 1 distinct candidate\(s\) of 24 draws"):
        sampler.sample(raw, keys=[5, 77])


def test_ids_outside_their_range_are_refused_before_any_launch(images, sampler):
    bad = dict(images[0], rel_ind=np.array([[0, 36]], np.int64), pred_dist=images[0]["pred_dist"][:1])
    with pytest.raises(ValueError, match=r"relation endpoints must lie in \[0, 36\), got values from 0 to 36"):
        sampler.sample(_raw([bad]))
    bad = dict(images[0], rel_ind=np.array([[-1, 3]], np.int64), pred_dist=images[0]["pred_dist"][:1])
    with pytest.raises(ValueError, match=r"relation endpoints must lie in \[0, 36\), got values from -1 to 3"):
        sampler.extract(_raw([bad]), np.array([1], np.uint64), [0, 1])
    with pytest.raises(ValueError, match=r"built for 64 objects per image \(obj_num - 1\), got 36"):
        P.ProposalSampler(4, obj_num=65).sample(_raw(images))
    with pytest.raises(ValueError, match=r"0 <= key < 2\^43 = 8796093022208, got -3"):
        sampler.sample(_raw(images), keys=[1, 2, -3])
    with pytest.raises(ValueError, match=r"U \[3, 24, 36\] and w \[3, 24\], got \(3, 24, 35\) and \(3, 24\)"):
        sampler.sample(_raw(images), uniforms=(np.zeros((3, 24, 35), np.float32), np.zeros((3, 24), np.float32)))


# ---- 4. two routes, one result ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def route_b(images, sampler, drawn):
    """The sampler's kept candidates copied to the host and fed back through `assemble_test_batch` as precomputed ones."""
    cand = sampler.train_candidates(drawn)
    host = {k: (v.cpu().numpy().copy() if torch.is_tensor(v) else list(v)) for k, v in cand.items()}
    raw = _raw(images)
    raw.update({k: (torch.from_numpy(v).to(DEV) if isinstance(v, np.ndarray) else v) for k, v in host.items()})
    return CI.assemble_test_batch(raw, OBJ, REL), host


def test_items_equal_those_of_the_test_loader_fed_with_the_kept_candidates(drawn, route_b, restated):
    items, host = route_b
    assert host["cand_node_mask"].shape == (int(drawn.table["kept"].sum()), OBJ - 1) and host["cand_pred_mask"].shape[1] == REL - 1
    assert host["cand_off"] == drawn.table["off"].tolist() and host["cand_nrel"].shape[0] == host["cand_nrel_off"][-1]
    for b, (a, want) in enumerate(zip(drawn.items, items)):
        assert set(a) == set(want) and a["this_mini_batch"] == want["this_mini_batch"]
        for k in ITEM_KEYS:
            assert a[k].shape == want[k].shape and a[k].dtype == want[k].dtype and torch.equal(a[k], want[k]), (b, k)
        r, mb = restated[b], a["this_mini_batch"]                                                # and both equal the numpy chain's rows
        for k in G.ROWS:
            rows = r["rows"][k][r["kept"][:2 * mb]].reshape(2, mb, *r["rows"][k].shape[1:])
            assert a[k].shape[0] == 5 and np.array_equal(a[k][0].cpu().numpy(), rows) and np.array_equal(a[k][4].cpu().numpy(), rows), (b, k)


def _same_entry(p, q, keys=()):
    assert p["image_id"] == q["image_id"] and p["caption"] == q["caption"]
    assert p["subgraph_score"].tobytes() == q["subgraph_score"].tobytes()
    np.testing.assert_array_equal(p["sorted_subgraph_ind"], q["sorted_subgraph_ind"])
    for k in keys:
        for f in p[k]:
            assert np.array_equal(np.asarray(p[k][f]), np.asarray(q[k][f])), (k, f)


@pytest.mark.parametrize("kw", [dict(sample_max=1, beam_size=1), dict(sample_max=1, beam_size=2, return_att=1)], ids=["greedy", "beam2_att"])
def test_caption_scene_graphs_equals_caption_images_on_the_other_routes_items(model, images, sampler, drawn, route_b, kw):
    infos = [{"id": i} for i in IDS]
    got = eval_glue.caption_scene_graphs(model, _raw(images), infos, VOCAB, sampler, kw)
    want = eval_glue.caption_images(model, route_b[0], infos, VOCAB, kw)
    t = drawn.table
    for b, (p, q) in enumerate(zip(got, want)):
        _same_entry(p, q, ("grounding",) if "return_att" in kw else ())
        assert set(p) - set(q) == {"proposal"} and len(p["caption"]) >= 1
        rows = t["off"][b] + p["sorted_subgraph_ind"]
        assert p["proposal"]["node_mask"].dtype == np.uint64 and p["proposal"]["seed_mask"].dtype == np.uint64
        assert p["proposal"]["node_mask"].tolist() == t["node_mask"][rows].tolist() and p["proposal"]["seed_mask"].tolist() == t["seed_mask"][rows].tolist()
        assert (p["sorted_subgraph_ind"] < t["used"][b]).all()
        assert all(int(s) & ~int(n) == 0 for s, n in zip(p["proposal"]["seed_mask"], p["proposal"]["node_mask"]))   # seeds are nodes of their sub-graph
    assert len({c for p in got for c in p["caption"]}) > 1


def test_sct_models_are_refused(model, images, sampler):
    with pytest.raises(ValueError, match="sct = 1"):
        eval_glue.caption_scene_graphs(model, _raw(images), [{"id": i} for i in IDS], VOCAB, sampler, dict(sct=1))


# ---- 5. batching cannot change an image ---------------------------------------------------------------------------------------------------

def test_batch_composition_order_and_group_do_not_change_an_image(model, images, sampler):
    kw = dict(sample_max=1, beam_size=1)
    run = lambda order, **k: {p["image_id"]: p for p in eval_glue.caption_scene_graphs(model, _raw([images[i] for i in order]), [{"id": IDS[i]} for i in order],
                                                                                       VOCAB, sampler, kw, **k)}
    together = run([0, 1, 2])
    alone = {}
    for i in range(3):
        alone.update(run([i]))
    for other in (alone, run([2, 1, 0]), run([0, 1, 2], group=1), run([0, 1, 2], group=256)):
        assert set(other) == set(together)
        for k, p in together.items():
            _same_entry(p, other[k], ("proposal",))


# ---- 6. node IoU ------------------------------------------------------------------------------------------------------------------------------

def test_node_iou_counts_and_quotients_equal_the_restatement(sampler, drawn):
    rng = np.random.default_rng(11)
    gt = (rng.random((3, 5, OBJ - 1)) < 0.2).astype(np.uint8)
    gt[1, 2] = 0                                                                                # a sentence that matched no noun
    gt[0, 0] = ((drawn.table["node_mask"][0] >> np.arange(OBJ - 1, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)   # ... and one equal to a candidate
    iou, inter, union = sampler.node_iou(drawn, torch.from_numpy(gt).to(DEV), counts=True)
    t = drawn.table
    for b in range(3):
        ri, ru, rq = P.restate_node_iou(gt[b], t["node_mask"][t["off"][b]:t["off"][b + 1]])
        assert inter[b].dtype == np.int64 and iou[b].dtype == np.float64 and iou[b].shape == (5, 5 + t["kept"][b])
        assert np.array_equal(inter[b], ri) and np.array_equal(union[b], ru) and iou[b].tobytes() == rq.tobytes(), b
        diag = np.diag(iou[b][:, :5])
        assert diag.tolist() == [0.0 if not gt[b, s].any() else 1.0 for s in range(5)]            # the sentences' own sets: diagonal 1
    assert iou[0][0, 5] == 1.0 and sampler.node_iou(drawn, torch.from_numpy(gt).to(DEV))[2].tobytes() == iou[2].tobytes()
    from subgc.assemble import choose_subgraphs
    ids = choose_subgraphs(iou[0], 0.5, 2, np.random.RandomState(0))                            # the table is what the host-side choice reads
    assert ids.shape == (5, 2, 2) and ids.min() >= 0 and ids.max() < 5 + t["kept"][0]
    with pytest.raises(ValueError, match=r"gt_node_mask \[3, 5, 36\], got \(3, 4, 36\)"):
        sampler.node_iou(drawn, torch.zeros(3, 4, 36, dtype=torch.uint8, device=DEV))


# ---- 7. no output element is left unwritten -----------------------------------------------------------------------------------------------

def test_no_output_element_is_left_unwritten(images, sampler, drawn, monkeypatch):
    """Every buffer of the chain starts as a sentinel (NaN / 0x3fffffff / 255): none survives in an output, and the results are the plain run's."""
    real = torch.empty

    def poisoned(*a, **k):
        t = real(*a, **k)
        if t.is_cuda and t.numel():
            t.fill_(float("nan")) if t.is_floating_point() else t.fill_(0x3fffffff if t.dtype != torch.uint8 else 255)
        return t
    raw = _raw(images)
    monkeypatch.setattr(torch, "empty", poisoned)
    try:
        seed, U, w = sampler.draw_seeds(3, OBJ - 1, IDS, DEV)
        got = sampler.sample(raw, keys=IDS)
        cand = sampler.train_candidates(got)
        rows = sampler.extract(raw, seed, [0, N_DRAW, 2 * N_DRAW, 3 * N_DRAW])
    finally:
        monkeypatch.setattr(torch, "empty", real)
    outs = [("seed", seed), ("U", U), ("w", w)] + [(f"cand {k}", v) for k, v in cand.items() if torch.is_tensor(v)] + [(f"rows {k}", v) for k, v in rows.items()]
    for b, it in enumerate(got.items):
        outs += [(f"item {b} {k}", it[k]) for k in ITEM_KEYS]
    for name, t in outs:
        t = t.cpu()
        assert not (torch.isnan(t).any() if t.is_floating_point() else (t == (255 if t.dtype == torch.uint8 else 0x3fffffff)).any()), name
    for k in drawn.table:
        assert np.array_equal(got.table[k], drawn.table[k]), k
    for a, b in zip(got.items, drawn.items):
        for k in ITEM_KEYS:
            assert torch.equal(a[k], b[k]), k
