"""Sub-graph proposals (subgc.proposals): the numpy restatements of the seed, expansion, duplicate-removal and node-IoU contracts on a
graph worked by hand, the sampler's option limits, and the stream property of the seed draw.  The device path is compared with these
restatements in tests/test_proposals_gpu.py."""
import numpy as np
import pytest

from subgc import proposals as P

# six nodes; nodes 0 and 1 share a class; the relations form the chain 2 - 3 - 4; node 5 stands alone.  obj_num 7, rel_num 5.
CLS = np.array([0, 0, 1, 2, 3, 4])
DIST = np.eye(6, dtype=np.float32)[CLS] * 0.5 + 0.05
REL = np.array([[2, 3], [3, 4]], np.int64)
SEEDS = np.array([1 << 0, 1 << 1, 1 << 2, 1 << 3, 1 << 4, 1 << 5], np.uint64)
# by hand: {0} and {1} both grow to their class {0, 1}; {2} takes relation 0 and its other end; {3} takes both relations; {4} takes
# relation 1 (the chain is followed one step, not to its end); {5} touches nothing
NODES = [[0, 1], [0, 1], [2, 3], [2, 3, 4], [3, 4], [5]]
RELS = [[], [], [0], [0, 1], [1], []]
NREL = [[], [], [[0, 1]], [[0, 1], [1, 2]], [[0, 1]], []]


def test_extraction_of_the_hand_worked_graph():
    rows = P.restate_extract(SEEDS, DIST, REL, 7, 5)
    assert rows["object_cls"].tolist() == CLS.tolist()
    for j in range(6):
        assert rows["gpn_obj_ind"][j].tolist() == NODES[j] + [6] * (7 - len(NODES[j]))
        assert rows["att_masks"][j].tolist() == [1.0] * len(NODES[j]) + [0.0] * (7 - len(NODES[j]))
        assert np.array_equal(rows["gpn_pool_mtx"][j], np.diag(rows["att_masks"][j]))
        assert rows["gpn_pred_ind"][j].tolist() == RELS[j] + [4] * (5 - len(RELS[j]))
        assert rows["gpn_nrel_ind"][j].tolist() == NREL[j] + [[6, 6]] * (5 - len(NREL[j]))
        assert int(rows["node_mask"][j]) == sum(1 << v for v in NODES[j])


def test_duplicate_removal_keeps_the_first_and_an_odd_last_survivor_is_not_used():
    node = P.restate_extract(SEEDS, DIST, REL, 7, 5)["node_mask"]
    kept, used = P.restate_dedup(node)
    assert kept.tolist() == [0, 2, 3, 4, 5] and used == 4                          # candidate 1 repeats candidate 0; five survivors, four used
    kept, used = P.restate_dedup(np.array([5, 5, 5, 5], np.uint64))
    assert kept.tolist() == [0] and used == 0
    kept, used = P.restate_dedup(np.array([1 << 63, 1, 1 << 63, 3], np.uint64))    # bit 63 is a node like any other
    assert kept.tolist() == [0, 1, 3] and used == 2


def test_seeds_from_injected_uniforms_by_hand():
    U = np.array([[0.5, 0.9, 0.9, 0.1, 0.2, 0.3],          # w 0.5 -> s = 1 + floor(1.5) = 2: columns 1 and 2 (equal values: the lower first)
                  [0.5, 0.9, 0.9, 0.1, 0.2, 0.3],          # w 0.0 -> s = 1: of the two equal maxima the LOWER column, 1
                  [0.5, 0.9, 0.9, 0.1, 0.2, 0.3],          # w 1.0 -> floor(3.0) = 3 is clamped to s_hi - s_lo = 2: s = 3, columns 1, 2, 0
                  [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]], np.float32)   # all equal, w just below 1 -> s = 3: columns 0, 1, 2
    w = np.array([0.5, 0.0, 1.0, np.float32(1) - np.float32(2.0 ** -24)], np.float32)
    mask, s, _, _ = P.restate_seeds(4, 6, (1, 3), 2019, 0, U=U, w=w)
    assert s.tolist() == [2, 1, 3, 3] and mask.tolist() == [0b110, 0b010, 0b111, 0b111]
    mask, s, _, _ = P.restate_seeds(4, 6, (2, 2), 2019, 0, U=U, w=w)               # a range of one value: w does not matter
    assert s.tolist() == [2, 2, 2, 2] and mask.tolist() == [0b110, 0b110, 0b110, 0b011]


def test_the_stream_is_a_function_of_seed_key_candidate_and_column():
    assert P.KEY_STRIDE > P.MAX_N * (64 + 1) and P.KEY_STRIDE >= P.MAX_N * P.ROW_PITCH and P.ROW_PITCH > P.W_COLUMN >= 64
    assert P.KEY_STRIDE % 4 == 0 and P.ROW_PITCH % 4 == 0                          # the uniform kernel starts at multiples of 4
    u0, w0 = P.stream_offsets(0, P.MAX_N, 64)
    u1, w1 = P.stream_offsets(1, P.MAX_N, 64)
    assert max(int(u0.max()), int(w0.max())) < min(int(u1.min()), int(w1.min()))   # two keys never share an offset, at the largest shape
    assert not np.intersect1d(u0[:4].ravel(), w0[:4]).size
    top_u, top_w = P.stream_offsets(P.MAX_KEY - 1, P.MAX_N, 64)
    assert int(top_w.max()) < 1 << 64 and int(top_w.max()) == (P.MAX_KEY - 1) * P.KEY_STRIDE + (P.MAX_N - 1) * P.ROW_PITCH + 64
    u = P.restate_uniform(2019, np.arange(4096, dtype=np.uint64))
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all() and 0.45 < float(u.mean()) < 0.55 and np.unique(u).size > 4000
    assert np.array_equal(P.restate_uniform(2019, np.arange(8, 24, dtype=np.uint64)), u[8:24])      # an offset names one value
    assert not np.array_equal(P.restate_uniform(2020, np.arange(16, dtype=np.uint64)), u[:16])


def test_an_images_seeds_do_not_depend_on_the_batch():
    """The restated draw of the images of a batch, keyed 3, 10 and 7: alone, together, reversed and beside strangers."""
    draw = lambda keys: {k: P.restate_seeds(24, 36, (1, 3), 2019, k)[0].tolist() for k in keys}
    alone = {k: draw([k])[k] for k in (3, 10, 7)}
    assert draw([3, 10, 7]) == alone and draw([7, 10, 3]) == alone
    assert {k: v for k, v in draw([99, 7, 0, 3, 10]).items() if k in alone} == alone
    assert alone[3] != alone[7] and alone[7] != alone[10]
    assert P.restate_seeds(24, 36, (1, 3), 2020, 3)[0].tolist() != alone[3]
    m, s, U, _ = P.restate_seeds(24, 36, (1, 3), 2019, 3)
    assert all(bin(int(v)).count("1") == int(k) for v, k in zip(m, s)) and set(s.tolist()) <= {1, 2, 3} and len(set(s.tolist())) > 1
    assert all(int(v) >> int(np.argmax(U[j])) & 1 for j, v in enumerate(m))         # the largest uniform's column is always a seed
    # a longer draw of the same image starts with the shorter one: candidate j does not depend on n
    assert P.restate_seeds(48, 36, (1, 3), 2019, 3)[0][:24].tolist() == alone[3]


def test_node_iou_by_hand():
    gt = np.zeros((5, 6), np.uint8)
    gt[0, [0, 1]] = 1
    gt[1, [2, 3]] = 1
    gt[3, :] = 1                                                                   # sentence 2 matched no noun: the empty set
    gt[4, 5] = 1
    kept = np.array([3, 12, 28, 24, 32], np.uint64)                                # {0,1} {2,3} {2,3,4} {3,4} {5}
    inter, union, iou = P.restate_node_iou(gt, kept)
    assert inter.shape == union.shape == iou.shape == (5, 10) and iou.dtype == np.float64
    assert np.diag(iou[:, :5]).tolist() == [1.0, 1.0, 0.0, 1.0, 1.0]               # both sets empty: 0 by definition (the reference divides by zero)
    assert iou[0, 5:].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]
    assert iou[1, 5:].tolist() == [0.0, 1.0, 2 / 3, 1 / 3, 0.0]
    assert not iou[2].any() and inter[2].tolist() == [0] * 10 and union[2].tolist() == [2, 2, 0, 6, 1, 2, 2, 3, 2, 1]
    assert iou[3, 5:].tolist() == [2 / 6, 2 / 6, 3 / 6, 2 / 6, 1 / 6] and iou[3, :5].tolist() == [2 / 6, 2 / 6, 0.0, 1.0, 1 / 6]
    assert inter[1, 7] == 2 and union[1, 7] == 3 and np.array_equal(iou[:, :5], iou[:, :5].T)


@pytest.mark.parametrize("kw, text", [
    (dict(n=0), r"2 <= n <= 8192 .*got 0"),
    (dict(n=7), r"n must be even .*got 7"),
    (dict(n=8194), r"2 <= n <= 8192 .*got 8194"),
    (dict(n=4, seeds=(0, 3)), r"1 <= s_lo <= s_hi <= 32 = min\(32, obj_num - 1\).*got \(0, 3\)"),
    (dict(n=4, seeds=(3, 2)), r"1 <= s_lo <= s_hi <= 32 .*got \(3, 2\)"),
    (dict(n=4, seeds=(1, 33)), r"s_hi <= 32 = min\(32, obj_num - 1\).*k <= 32.*got \(1, 33\)"),
    (dict(n=4, seeds=(1, 7), obj_num=7), r"s_hi <= 6 = min\(32, obj_num - 1\).*got \(1, 7\)"),
    (dict(n=4, seeds=(1, 2, 3)), r"seeds = \(s_lo, s_hi\), got \(1, 2, 3\)"),
    (dict(n=4, obj_num=66), r"obj_num - 1 <= 64 objects per image .*got obj_num = 66"),
    (dict(n=4, obj_num=1), r"got obj_num = 1"),
    (dict(n=4, rel_num=1), r"2 <= rel_num <= 1024, got 1"),
    (dict(n=4, rel_num=1025), r"2 <= rel_num <= 1024, got 1025"),
    (dict(n=4, seed=-1), r"0 <= seed < 2\^64, got -1"),
])
def test_every_limit_is_refused_with_its_number(kw, text):
    with pytest.raises(ValueError, match=text):
        P.ProposalSampler(**kw)


def test_limits_that_are_allowed_and_keys():
    s = P.ProposalSampler(8192, seeds=(32, 32), obj_num=65, rel_num=1024, seed=(1 << 64) - 1)
    assert (s.n, s.seeds, s.obj_num) == (8192, (32, 32), 65)
    s = P.ProposalSampler(2, seeds=(1, 1), obj_num=2, rel_num=2)
    assert s._keys(None, 3) == [0, 1, 2] and s._keys([5, np.int64(9), (1 << 43) - 1], 3) == [5, 9, (1 << 43) - 1]
    for bad, text in ((-1, "got -1"), (1 << 43, f"got {1 << 43}"), (1.5, "got 1.5"), ("7", "got '7'"), (True, "got True")):
        with pytest.raises(ValueError, match=r"0 <= key < 2\^43 = 8796093022208, " + text):
            s._keys([0, bad], 2)
    with pytest.raises(ValueError, match="3 keys for 2 images"):
        s._keys([1, 2, 3], 2)


def test_image_ids_become_keys_without_the_batch():
    from subgc.eval_glue import proposal_key
    assert proposal_key(391895) == 391895 and proposal_key(np.int64(7)) == 7 and proposal_key(0) == 0
    assert proposal_key("COCO_val2014_000000391895.jpg") == proposal_key("COCO_val2014_000000391895.jpg") < 1 << 32
    assert proposal_key("a") != proposal_key("b") and 0 <= proposal_key(-5) < 1 << 32 and 0 <= proposal_key(1 << 50) < 1 << 32
