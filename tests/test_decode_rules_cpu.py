"""Decode rules without a GPU: the restatement on hand-worked rows, `DecodeRules.from_options`, the fourteenth header's pin, the
untouched post-hoc `remove_bad_endings`, and the CPU oracle driven step by step under all four rules on the golden tiny models (the
fixture check of the GPU test: at most 5 % of its steps may have a ruled top-2 gap below 1e-3)."""
import math
import os
import re

import numpy as np
import pytest
import torch

import decode_rules_reference as R
from subgc import _lib, eval_glue
from subgc.decode_rules import BEAM_REFUSED, DecodeRules, apply_rules_restatement, bad_ending_ids, trigram_counts

PEN = float(np.float32(np.float32(-0.693) * np.float32(2.0)))
IX = {str(i): w for i, w in enumerate(["<eos>", "a", "dog", "on", "grass", "with", "the", "UNK"])}


def _lp(x):
    x = np.asarray(x, np.float64)
    return x - x.max() - math.log(np.exp(x - x.max()).sum())


def test_one_earlier_trigram_blocks_its_third_word_with_count_one():
    x = np.linspace(-1, 1, 9)
    tri = DecodeRules(block_trigrams=1)
    assert tri.active and tri.flags == 1 and float(tri.trigram_pen) == PEN and abs(PEN + 1.386) < 1e-6
    h = [1, 2, 3, 1, 2, 0, 0]
    assert trigram_counts(h, 5, 9) == {3: 1}
    got, ev = apply_rules_restatement(x, h, 5, tri, return_events=True)
    want = _lp(x)
    want[3] += 1.0 * PEN
    np.testing.assert_array_equal(got, want)
    assert ev.tolist() == [[1, 0, 0, 0]]                                       # column 8 stays the arg-max


def test_a_a_a_a_counts_two_at_step_four():
    x = np.zeros(8)
    assert trigram_counts([5, 5, 5, 5], 4, 8) == {5: 2}
    got, ev = apply_rules_restatement(x, [5, 5, 5, 5], 4, DecodeRules(block_trigrams=1), return_events=True)
    want = _lp(x)
    want[5] += 2.0 * PEN
    np.testing.assert_array_equal(got, want)
    assert ev.tolist() == [[1, 0, 0, 0]]                                       # ties: the first arg-max is column 0 before and after
    got5 = apply_rules_restatement(x, [0, 0, 0, 0], 4, DecodeRules(block_trigrams=1), return_events=True)
    assert got5[1].tolist() == [[1, 0, 0, 1]] and got5[0].argmax() == 1        # ... and moves when column 0 is the one counted


@pytest.mark.parametrize("t", [0, 1, 2])
def test_fewer_than_three_tokens_give_no_trigram(t):
    x = np.arange(8.0)
    got, ev = apply_rules_restatement(x, [3, 3, 3, 3], t, DecodeRules(block_trigrams=1), return_events=True)
    np.testing.assert_array_equal(got, _lp(x))
    assert not ev.any() and trigram_counts([3, 3, 3, 3], t, 8) == {}


def test_alpha_inf_is_a_hard_block_on_counted_columns_only_and_no_nan():
    r = DecodeRules(block_trigrams=1, trigram_alpha=float("inf"))
    assert float(r.trigram_pen) == -math.inf
    x = np.stack([np.linspace(-2, 2, 10), np.zeros(10)])
    h = np.array([[1, 2, 3, 1, 2], [4, 4, 4, 4, 4]])
    got = apply_rules_restatement(x, h, 5, r)
    assert not np.isnan(got).any()
    assert np.argwhere(np.isinf(got)).tolist() == [[0, 3], [1, 4]] and (got[np.isinf(got)] < 0).all()
    keep = np.ones_like(got, bool)
    keep[0, 3] = keep[1, 4] = False
    np.testing.assert_array_equal(got[keep], np.stack([_lp(x[0]), _lp(x[1])])[keep])
    assert float(DecodeRules(block_trigrams=1, trigram_alpha=0.0).trigram_pen) == 0.0


def test_the_repeat_ban_does_nothing_at_step_zero_and_bans_the_last_word_after():
    x = np.arange(8.0)
    rep = DecodeRules(decoding_constraint=1)
    got0, ev0 = apply_rules_restatement(x, [7, 7], 0, rep, return_events=True)
    np.testing.assert_array_equal(got0, _lp(x))
    assert not ev0.any()
    got1, ev1 = apply_rules_restatement(x, [7, 7], 1, rep, return_events=True)
    assert got1[7] == -math.inf and np.isfinite(got1[:7]).all() and ev1.tolist() == [[0, 1, 0, 1]]
    np.testing.assert_array_equal(got1[:7], _lp(x)[:7])


def test_a_bad_ending_bans_the_end_token_only_after_a_listed_id():
    bad = DecodeRules(block_bad_endings=1, bad_ids=(3, 5))
    x = np.array([3.0, 0, 0, 0, 0, 0, 0, 1.0])
    for last, hit in ((3, True), (5, True), (4, False), (0, False)):
        got, ev = apply_rules_restatement(x, [1, last], 2, bad, return_events=True)
        assert (got[0] == -math.inf) == hit and np.isfinite(got[1:]).all()
        assert ev.tolist() == [[0, 0, int(hit), int(hit)]]
        np.testing.assert_array_equal(got[1:], _lp(x)[1:])
    got0 = apply_rules_restatement(x, [3, 3], 0, bad)                            # no history yet
    np.testing.assert_array_equal(got0, _lp(x))


def test_the_unk_penalty_and_the_order_of_the_rules_on_one_column():
    x = np.zeros(8)
    allr = DecodeRules(block_trigrams=1, suppress_unk=1, decoding_constraint=1, block_bad_endings=1, bad_ids=(7,))
    assert allr.flags == 15
    got, ev = apply_rules_restatement(x, [7, 7, 7, 6], 3, allr, return_events=True)       # h = 7 7 7: count 1 on 7, UNK = 7, last = 7
    assert got[7] == -math.inf and got[0] == -math.inf and ev.tolist() == [[1, 1, 1, 1]]
    got2 = apply_rules_restatement(x, [7, 7, 7, 6], 3, DecodeRules(block_trigrams=1, suppress_unk=1))
    assert got2[7] == (_lp(x)[7] + 1.0 * PEN) - 1000.0


def test_from_options_defaults_keys_and_refusals():
    r = DecodeRules.from_options({})
    assert r == DecodeRules() and not r.active and r.key is None and r.flags == 0 and r.trigram_alpha == 2.0
    assert DecodeRules.from_options(None) == r and DecodeRules.from_options({"remove_bad_endings": 1}) == r
    on = DecodeRules.from_options({"block_trigrams": 1, "block_bad_endings": 1, "suppress_unk": 1, "decoding_constraint": 1}, IX)
    assert on.active and on.flags == 15 and on.bad_ids == (1, 3, 5, 6) == bad_ending_ids(IX)
    assert hash(on.key) == hash(DecodeRules.from_options({"block_trigrams": 1, "block_bad_endings": 1, "suppress_unk": 1,
                                                          "decoding_constraint": 1, "bad_ending_ids": [1, 3, 5, 6]}).key)
    assert on.key != DecodeRules.from_options({"block_trigrams": 1, "trigram_alpha": 3.0}).key
    assert DecodeRules.from_options({"block_trigrams": 1, "trigram_alpha": 3.0}).trigram_pen == np.float32(np.float32(-0.693) * np.float32(3.0))
    with pytest.raises(ValueError, match="trigram_alpha = -1"):
        DecodeRules.from_options({"block_trigrams": 1, "trigram_alpha": -1})
    with pytest.raises(ValueError, match="trigram_alpha"):
        DecodeRules(trigram_alpha=float("nan"))
    with pytest.raises(ValueError, match="65 ids"):
        DecodeRules.from_options({"block_bad_endings": 1, "bad_ending_ids": list(range(65))})
    DecodeRules.from_options({"block_bad_endings": 1, "bad_ending_ids": list(range(64))})
    with pytest.raises(ValueError, match="bad_ending_ids"):
        DecodeRules.from_options({"block_bad_endings": 1})
    for name in BEAM_REFUSED:
        with pytest.raises(ValueError, match=f"^{name} = 1 with beam_size = 3"):
            DecodeRules.from_options({name: 1, "beam_size": 3, "bad_ending_ids": [1]})
    assert not DecodeRules.from_options({"decoding_constraint": 1, "beam_size": 3}).active     # beam search keeps its own meaning of it
    assert DecodeRules.from_options({"decoding_constraint": 1, "beam_size": 1}).flags == 4


def test_the_fourteenth_header_declares_one_entry_point_and_nobody_else_does():
    assert list(_lib.HEADERS)[-1] == "decode_rules" and len(_lib.HEADERS) == 14
    assert os.path.basename(_lib.DECODE_RULES_HEADER) == "subgc_decode_rules_hip.h" and callable(_lib.call_decode_rules)
    protos = _lib.parse_header(_lib.DECODE_RULES_HEADER)
    assert set(protos) == {"subgc_decode_rules"}
    assert [a for _, a in protos["subgc_decode_rules"][1]] == ["logits", "ld", "n", "V", "seq", "T", "t", "flags", "trigram_pen", "bad_ids",
                                                               "n_bad", "stats", "prev_count", "stream"]
    inc = os.path.dirname(_lib.HEADER)
    for key, hdr in _lib.HEADERS.items():
        if key != "decode_rules":
            assert "subgc_decode_rules" not in _lib.parse_header(os.path.join(inc, hdr)), hdr
    assert len(_lib.parse_header(_lib.HEADER)) == 133                            # the core header keeps its entry points
    src = open(_lib.DECODE_RULES_HEADER).read()
    consts = dict(re.findall(r"#define (SUBGC_RULE\w*) (\d+)", src))
    assert (consts["SUBGC_RULES_MAX_V"], consts["SUBGC_RULES_MIN_V"], consts["SUBGC_RULES_MAX_T"], consts["SUBGC_RULES_MAX_BAD"]) == ("16384", "8", "64", "64")
    assert [consts[k] for k in ("SUBGC_RULE_TRIGRAMS", "SUBGC_RULE_UNK", "SUBGC_RULE_REPEAT", "SUBGC_RULE_BAD_END")] == ["1", "2", "4", "8"]
    L = _lib.lib()
    assert hasattr(L, "subgc_decode_rules")


def test_remove_bad_endings_still_trims_the_finished_strings():
    seq = [[2, 3, 6, 0, 0], [2, 3, 4, 5, 0], [1, 6, 0, 0, 0]]
    assert eval_glue.decode_sequence(IX, seq, 0) == ["dog on the", "dog on grass with", "a the"]
    assert eval_glue.decode_sequence(IX, seq, 1) == ["dog", "dog on grass", "a the"]   # (misc/utils.py:74-79: all bad endings -> kept)
    assert eval_glue.BAD_ENDINGS == ("with", "in", "on", "of", "a", "at", "to", "for", "an", "this", "his", "her", "that", "the")


def test_the_bound_adds_one_rounding_per_operation():
    x = np.linspace(-3, 3, 37)
    h = [1, 2, 36, 1, 2]
    plain = R.ruled_bound(x, h, 5, DecodeRules())
    both = R.ruled_bound(x, h, 5, DecodeRules(block_trigrams=1, suppress_unk=1))
    lp = _lp(x)
    np.testing.assert_array_equal(both[:36], plain[:36])
    v1 = lp[36] + PEN
    assert both[36] == pytest.approx(plain[36] + 1.001 * R.U * (abs(PEN) + abs(v1) + abs(v1 - 1000.0)), rel=1e-12)
    assert plain.max() < 2e-6 and both[36] < 7e-5


def test_every_history_kind_is_what_its_name_says():
    V, T = 37, 20
    for t in (4, 19):
        c = [trigram_counts(R.history(k, T, t, V), t, V) for k in R.KINDS]
        assert c[0] == {} and c[3] == {3: 1} and c[4] == {0: t - 2}
        assert sum(c[1].values()) == 1
    assert trigram_counts(R.history("multiplicity 3", T, 19, V), 19, V) == {5: 5} and trigram_counts(R.history("multiplicity 3", 64, 11, V), 11, V) == {6: 3}
    assert V - 1 in trigram_counts(R.history("id V-1", T, 19, V), 19, V) or 2 in trigram_counts(R.history("id V-1", T, 19, V), 19, V)
    assert (R.history("zeros", T, 5, V)[5:] == V - 1).all()


def test_the_markov_cycle_breaks_at_step_five_on_the_host():
    tab = R.markov_tables(3, 12, seed=1)
    step = lambda it: tab[np.arange(3), it]
    plain, _, s0, _ = R.host_loop(step, 3, 12, DecodeRules())
    assert plain[0].tolist() == [1, 2, 3] * 4 and not s0.any()
    seq, lps, stats, gap = R.host_loop(step, 3, 12, DecodeRules(block_trigrams=1))
    assert seq[0, :5].tolist() == [1, 2, 3, 1, 2] and seq[0, 5] == 4 and stats[0, 0] >= 1 and stats[0, 3] >= 1
    assert gap >= 1e-3                                                           # the fixture leaves no near-tie to the fp32 device


# ------------------------------------------------------------------------------------------------ the golden tiny models under the rules
@pytest.mark.parametrize("name", ["subgc", "fullgc"])
def test_the_cpu_oracle_under_all_rules_stays_clear_of_near_ties(golden, name):
    """The share of live steps whose ruled top-2 gap is below 1e-3 (printed; at most 5 % by the issue's cap), and at least one trigram
    hit, on the CPU oracle alone -- the fixture check of test_decode_rules_loop_gpu.py."""
    orc, opt, w, batches = R.oracle_case(golden, name)
    rules = R.all_rules(opt["vocab_size"] + 1)
    from subgc import synthetic
    near = total = hits = 0
    for tb in batches:
        a = synthetic.sample_args(tb)
        args = (a[0], a[1], a[2], a[4], a[6], a[8], a[9], a[12])
        seq, lps, stats, gaps, live_hits = R.oracle_ruled_greedy(orc, args, rules)
        near += int((gaps < 1e-3).sum()); total += gaps.size; hits += live_hits
    print(f"{name}: {near} of {total} live steps with a ruled top-2 gap < 1e-3 ({100.0 * near / total:.2f} %), {hits} trigram hits on live rows")
    assert total >= 10 and near <= 0.05 * total
    assert hits >= 1
