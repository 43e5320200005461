"""Self-critical sequence training without a GPU: the sixth header and its binding, the fixtures the reference's own RewardCriterion and COCO
scorers wrote (tests/golden/make_golden_self_critical.py) against the fp64 restatements the GPU tests use as their reference, the derived
bounds against the reference's own fp32 results, and every host-side refusal with its text."""
import argparse
import ctypes

import numpy as np
import pytest

import accuracy_golden as AG
import self_critical_golden as G
from subgc import _lib, ops, selfcritical
from subgc._lib import SubgcError
import subgc.models as models

NLL_EXTRA = ["reward", "r_stride"]
NAMES = {
    "subgc_sc_pick": ["logits", "ld", "n", "n_sample", "V", "temp", "u", "t", "seq", "seqlp", "T", "next_tok", "unfinished", "n_unfinished",
                      "prev_count", "raw_logits", "stream"],
    "subgc_sc_prepare": ["seq2", "S", "T", "V", "eos_id", "labels", "mask", "score_rows", "stream"],
    "subgc_sc_reward": ["row_d", "ld_d", "S", "T1", "w_cider", "w_bleu", "reward", "mean_reward", "scores", "stream"],
    "subgc_reward_nll_fwd": ["input", "seq", "reward", "gpn_loss", "loss", "scratch2", "S", "T", "stream"],
    "subgc_reward_nll_bwd": ["seq", "reward", "gpn_loss", "scratch2", "dloss", "dinput", "dgpn", "S", "T", "stream"],
    "subgc_reward_logits_fwd": ["logp", "target", "t_stride", "mask", "m_stride", "reward", "r_stride", "loss", "scratch2", "S", "T", "V",
                                "den_override", "lse", "stream"],
    "subgc_reward_logsoftmax_bwd": ["logp", "target", "t_stride", "mask", "m_stride", "reward", "r_stride", "scratch2", "dloss", "dlogits",
                                    "ld_out", "S", "T", "V", "active", "out_bf16", "lse", "stream"],
}


def test_selfcritical_header_parses_and_the_other_five_are_untouched():
    protos = _lib.parse_header(_lib.SELFCRITICAL_HEADER)
    assert sorted(protos) == sorted(NAMES)
    for name, want in NAMES.items():
        ret, args = protos[name]
        assert ret is ctypes.c_int and [a for _, a in args] == want, name
        assert dict((a, t) for t, a in args)["stream"] is ctypes.c_void_p
    assert dict((a, t) for t, a in protos["subgc_sc_reward"][1])["w_cider"] is ctypes.c_double
    # the fused forms = the NLL entry points' arguments plus the reward view; the pick = subgc_decode_pick's with n_sample for k
    core = _lib.parse_header()
    strip = lambda n: [a for a in NAMES[n] if a not in NLL_EXTRA]
    assert strip("subgc_reward_logits_fwd") == [a for _, a in core["subgc_masked_nll_fwd"][1]]
    assert strip("subgc_reward_logsoftmax_bwd") == [a for _, a in core["subgc_nll_logsoftmax_bwd"][1]]
    pick = [a for _, a in core["subgc_decode_pick"][1]]
    assert [a for a in NAMES["subgc_sc_pick"] if a != "n_sample"] == [("logits" if a == "logp" else a) for a in pick if a != "k"]
    src = open(_lib.SELFCRITICAL_HEADER).read()
    assert src.count("misc/utils.py:89-109") >= 5 and src.count("AttModel.py:295-316") >= 2 and src.count("opts.py:149-152") >= 1


def test_restated_criterion_reproduces_the_reference_class():
    """fp64 numpy against what misc/utils.py:89-109 computed in fp32: the loss within the derived bound (which the reference's own fp32
    result therefore meets: torch sums pairwise, no deeper than the kernel's order), the gradients to a few fp32 roundings."""
    meta, arr = G.load_case()
    seq = arr["seq"]
    assert seq.shape == arr["input"].shape == (meta["S"], meta["T"]) == (3, 5)
    assert not seq[meta["zero_row"]].any() and seq[meta["full_row"]].all() and seq[0, 2] > 0 and not seq[0, 3:].any()
    assert np.array_equal(G.mask_of(seq), [[1, 1, 1, 1, 0], [1, 0, 0, 0, 0], [1, 1, 1, 1, 1]])
    r_row = arr["reward_row"]
    assert (r_row[0] < 0).all() and not r_row[1].any() and (r_row[2] > 0).all() and np.ptp(arr["reward_tok"], axis=1).min() > 0
    assert meta["keys"] == ["row_plain", "row_gpn", "tok_plain", "tok_gpn"]
    for key in meta["keys"]:
        rname, gname = key.split("_")
        gpn = arr["gpn_loss"] if gname == "gpn" else None
        loss, dinp, dgpn = G.criterion64(arr["input"], seq, arr["reward_" + rname], gpn)
        bound = G.loss_bound(arr["input"], seq, arr["reward_" + rname], gpn)
        print(f"{key}: loss {loss:.9f} ref {float(arr['loss_' + key]):.9f} |d| {abs(loss - float(arr['loss_' + key])):.2e} bound {bound:.2e}")
        assert abs(loss - float(arr["loss_" + key])) <= bound, key
        np.testing.assert_allclose(arr["dinput_" + key], dinp, rtol=4 * G.U, atol=0, err_msg=key)
        if gpn is not None:
            np.testing.assert_allclose(arr["dgpn_" + key], dgpn, rtol=8 * G.U, atol=0, err_msg=key)
        else:
            assert "dgpn_" + key not in arr
    # a zero reward row contributes nothing and gets no gradient; the zero-seq row keeps exactly its first step
    _, dinp, _ = G.criterion64(arr["input"], seq, r_row)
    assert not dinp[1].any() and dinp[0, :4].all() and not dinp[0, 4]


def test_restated_end_token_rule_and_scores_reproduce_the_reference_scorers():
    """The fixture's strings were built as the upstream array_to_str builds them (the end token scored as a word).  Here the same rows go
    through the rule of subgc_sc_prepare -- first 0 -> eos_id, a row without a 0 untouched -- as id lists into the fp64 restatement of the
    COCO scorers: CIDEr and sentence BLEU-4 of all 2 x 20 rows within tests/accuracy_golden.py's bounds of the reference's values."""
    meta, arr = G.load_case()
    refs = G.per_image(arr["ref_rows"], arr["ref_cap_off"])
    assert len(refs) == meta["n_img"] == 12 and sorted({len(r) for r in refs}) == [1, 2, 3, 4, 5] and arr["cand"].shape == (40, meta["L"])
    cand = arr["cand"]
    for r in meta["empty_cands"]:
        assert not cand[r].any()
    for r in meta["full_cands"]:
        assert cand[r].all()
    img2 = np.concatenate([arr["cand_img"], arr["cand_img"]])
    for r, j, c in meta["equal_cands"]:
        assert img2[r] == j and np.array_equal(cand[r], refs[j][c])
    assert not refs[meta["empty_ref"][0]][meta["empty_ref"][1]].any() and refs[meta["full_ref"][0]][meta["full_ref"][1]].all()
    eos_id = meta["V"] + 1
    rows = G.eos_rows(cand, eos_id)
    assert rows.shape == (40, meta["L"] + 1) and rows[0, 0] == eos_id and not rows[0, 1:].any() and rows[1, -1] == 0 and rows[1, :-1].all()
    for r in range(40):
        assert [int(x) for x in rows[r] if x] == G.ids_with_eos(cand[r], eos_id)
    bleu4, cider = G.restate_scores(cand, img2, refs, eos_id)
    print(f"BLEU-4 rel {AG.rel(bleu4, arr['bleu'][:, 3]):.2e}  CIDEr rel {AG.rel(cider, arr['cider']):.2e}")
    assert AG.rel(bleu4, arr["bleu"][:, 3]) <= AG.BLEU_TOL and AG.rel(cider, arr["cider"]) <= AG.CIDER_TOL
    # the rule matters: without the end token the scores are other numbers
    b0, c0 = G.restate_scores(cand, img2, refs, 0)
    assert np.abs(c0 - arr["cider"]).max() > 1e-2
    # the replay's labels and mask of the first half
    lab, m = G.replay_labels(cand)
    assert lab.shape == (20, 12) and not lab[:, 0].any() and not lab[:, -1].any() and np.array_equal(lab[:, 1:-1], cand[:20])
    assert m.shape == (20, 11) and not m[:, -1].any() and m[:, 0].all() and np.array_equal(m[:, 1:10], cand[:20, :9] > 0)


def test_reward_references_cook_the_end_token_as_a_fresh_word():
    meta, arr = G.load_case()
    refs = G.per_image(arr["ref_rows"], arr["ref_cap_off"])
    r = selfcritical.RewardReferences(refs, device=None)
    assert r.eos_id == meta["V"] + 1 == r.n_ids and r.n_img == 12 and abs(r.ref_len - np.log(12.0)) < 1e-15
    assert r.word_to_ix["0"] == r.eos_id and r.word_to_ix["7"] == 7
    ldf, _ = AG.log_df([[G.ids_with_eos(c, r.eos_id) for c in caps] for caps in refs])
    assert len(ldf) == len(r.ukeys)                                             # the same distinct n-grams, the end token among them
    plain = selfcritical.RewardReferences(refs, eos=False, vocab_size=30, device=None)
    assert plain.eos_id == 0 and plain.n_ids == 30 and "0" not in plain.word_to_ix
    lab = np.concatenate([np.zeros((1, 10), np.int64)] + refs)                  # the loader's arrays: 1-based start, inclusive end
    start = arr["ref_cap_off"][:-1] + 2
    end = arr["ref_cap_off"][1:] + 1
    pick = [5, 0, 7]
    sub = selfcritical.RewardReferences.from_labels(lab[1:], start - 1, end - 1, pick, device=None)
    assert sub.n_img == 3 and sub.n_caps == sum(len(refs[j]) for j in pick)


def test_restated_pick_and_the_share_of_draws_near_a_boundary():
    assert G.inv_cdf_pick(np.log([0.2, 0.3, 0.5]), 0.0) == 0 and G.inv_cdf_pick(np.log([0.2, 0.3, 0.5]), 0.2) == 1
    assert G.inv_cdf_pick(np.log([0.2, 0.3, 0.5]), 0.4999) == 1 and G.inv_cdf_pick(np.log([0.2, 0.3, 0.5]), 0.999999) == 2
    onehot = np.full(9, -np.inf); onehot[4] = 0.0
    assert {G.inv_cdf_pick(onehot, u) for u in (0.0, 0.3, 1 - 2.0 ** -24)} == {4}
    assert G.inv_cdf_pick(np.log([0.5, 0.5]), 0.3, temp=0.5) == 0
    # a uniform draw lies within 1e-5 of one of the V - 1 inner boundaries with probability <= 2e-5 (V - 1): 1e-3 at the golden
    # vocabulary (V = 51), far below the 1 % of draws the rollout test may skip; measured here on seeded rows of that width
    rng = np.random.default_rng(5)
    near = sum(G.boundary_distance(rng.normal(size=51) * 2.0, rng.random()) < 1e-5 for _ in range(4000))
    assert near <= 0.01 * 4000 and 2e-5 * 50 < 0.01


def test_train_fixture_holds_losses_rewards_and_every_live_gradient(golden):
    z, base = G.load_train(), golden("subgc_train")
    grads = base.group("grads")
    extra = {k for k in z if k.startswith("sc.")}
    assert set(z) - extra == set(grads) | {"lang_loss", "gpn_loss", "loss"}
    assert extra == {"sc.seq2", "sc.ref_rows", "sc.ref_cap_off", "sc.gt_indices", "sc.weights", "sc.scores", "sc.reward", "sc.mean_reward"}
    assert all(z[k].shape == grads[k].shape and z[k].dtype == np.float32 for k in grads)
    out = base.group("out")
    assert float(z["gpn_loss"]) == float(out["gpn_loss"]) and float(z["lang_loss"]) != float(out["lang_loss"])     # only the language loss changed
    assert abs(float(z["lang_loss"]) + float(z["gpn_loss"]) - float(z["loss"])) < 1e-6
    seq2, b5 = z["sc.seq2"], z["sc.seq2"].shape[0] // 2
    assert seq2.shape == (30, 16) and not seq2[4].any() and seq2[6].all() and seq2.max() <= 50
    assert np.array_equal(z["sc.reward"], (z["sc.scores"][:b5] - z["sc.scores"][b5:]).astype(np.float32))
    assert (z["sc.reward"] > 0).any() and (z["sc.reward"] < 0).any()
    # the recorded scores are the restated scorers' on the end-token rows, with the weights of the fixture
    refs = G.per_image(z["sc.ref_rows"], z["sc.ref_cap_off"])
    img = np.concatenate([np.repeat(z["sc.gt_indices"], b5 // 3)] * 2)
    bleu4, cider = G.restate_scores(seq2, img, refs, 51)
    wc, wb = z["sc.weights"]
    np.testing.assert_allclose(wc * cider + wb * bleu4, z["sc.scores"], rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_reward_weights_that_are_not_finite_are_refused_with_their_value(bad):
    for wc, wb in ((bad, 0.0), (1.0, bad)):
        with pytest.raises(SubgcError) as e:
            ops.check_reward_weights(wc, wb)
        assert repr(float(bad)) in str(e.value) and "must be finite" in str(e.value)
        args = dict.fromkeys(NAMES["subgc_sc_reward"])
        args.update(ld_d=6, S=1, T1=1, w_cider=wc, w_bleu=wb)
        with pytest.raises(SubgcError, match="reward weights .* must be finite"):      # the library, before it looks at any pointer
            _lib.call_selfcritical("subgc_sc_reward", *args.values())
    refs = selfcritical.RewardReferences([np.array([[1, 2, 0]])], device=None)
    with pytest.raises(SubgcError, match="must be finite"):
        selfcritical.SelfCriticalReward(refs, cider_weight=bad)
    assert ops.check_reward_weights(1, 0) == (1.0, 0.0)


def test_host_side_refusals_fire_with_their_text():
    with pytest.raises(SubgcError, match=r"sc_flag=True needs a reward: build subgc.selfcritical.RewardReferences .*sc_reward=subgc.selfcritical.SelfCriticalReward"):
        models.LossWrapper(None, None).forward(*([None] * 17), sc_flag=True)
    with pytest.raises(SubgcError, match="sc_flag=True needs a reward"):
        models.LossWrapper(None, argparse.Namespace(label_smoothing=0.1))(*([None] * 17), sc_flag=True)
    refs = selfcritical.RewardReferences([np.array([[1, 2, 0]]), np.array([[3, 0, 0], [2, 2, 2]])], device=None)
    rw = selfcritical.SelfCriticalReward(refs, 1.0, 0.5)
    assert rw.check_index([1, 0, 1]) == [1, 0, 1]
    for bad in ([0, 2], [-1]):
        with pytest.raises(SubgcError, match=rf"batch image {len(bad) - 1} names reference image {bad[-1]}; the references hold 2 images"):
            rw.check_index(bad)
    with pytest.raises(SubgcError, match=r"rollouts of 64 steps are scored as rows of T \+ 1 = 65 words; the limit is 64"):
        rw.check_steps(64)
    rw.check_steps(63)
    with pytest.raises(SubgcError, match="references are a subgc.selfcritical.RewardReferences"):
        selfcritical.SelfCriticalReward(object())
    with pytest.raises(SubgcError, match="int array"):
        selfcritical.RewardReferences([np.array([[1.5, 2.0]])], device=None)
    # the library's own argument checks need no device either
    pick = dict.fromkeys(NAMES["subgc_sc_pick"])
    pick.update(ld=10, n=3, n_sample=4, V=10, temp=1.0, t=0, T=5, raw_logits=0)
    with pytest.raises(SubgcError, match=r"sc_pick: n_sample = 4 of n = 3 rows"):
        _lib.call_selfcritical("subgc_sc_pick", *pick.values())
    pick.update(n_sample=1, V=16385, ld=16385)
    with pytest.raises(SubgcError, match="sc_pick: at most 16384 columns"):
        _lib.call_selfcritical("subgc_sc_pick", *pick.values())


def test_loss_wrapper_keeps_its_signature_and_its_criteria():
    import inspect
    params = list(inspect.signature(models.LossWrapper.forward).parameters)
    assert len(params) == 1 + 17 + 1 and params[-1] == "sc_flag" and inspect.signature(models.LossWrapper.forward).parameters["sc_flag"].default is False
    lw = models.LossWrapper(None, None)
    assert type(lw.crit) is models.LanguageModelCriterion and lw.sc_reward is None
    assert list(inspect.signature(models.RewardCriterion.forward).parameters) == ["self", "input", "seq", "reward", "gpn_loss"]
