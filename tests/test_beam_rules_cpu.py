"""Beam search under decode rules without a GPU: the host `beam.search` with `rules=` over a stand-in decoder that walks a 4-word cycle
(beam_rules_fake), the counters of a beam (`sequence_events`), the -1-prefix argument of the device history layout pinned on the
restatement, and the parsing of `eval_kwargs["beam_rules"]`."""
import itertools
import math

import numpy as np
import pytest

import beam_rules_fake as FK
from subgc import beam
from subgc.decode_rules import DecodeRules, apply_rules_restatement, sequence_events

N_SUB, T, N, LENS = 3, 10, 5, (5, 2, 4)
SALTS = (0, 1, 2)
BAD = (1, 2, 3)
# kept beams (of n x beam per salt) of a PLAIN search that repeat a trigram, per (beam, group) over the three salts: the least seen with
# this recipe.  So a rules test cannot pass on a search that ignores its rules.
PLAIN_REPEATS = {(2, 1): (6, 6), (3, 1): (8, 9), (4, 2): (11, 12), (6, 3): (14, 18)}


def opt_of(beam_size, G, **beam_rules):
    o = dict(beam_size=beam_size, group_size=G, diversity_lambda=0.5)
    if beam_rules:
        o["beam_rules"] = beam_rules
    return o


def run(beam_size, G, salt, end_boost=0.0, **beam_rules):
    o = opt_of(beam_size, G, **beam_rules)
    rules = DecodeRules.from_beam_options(o)
    return beam.search(FK.HostEngine(N_SUB, beam_size, LENS, N, salt, end_boost), T, o, rules=rules), rules


def kept(done):
    return [(s, b, b["seq"].tolist()) for s, beams in enumerate(done) for b in beams]


def ends_badly(w):
    return 0 in w and w.index(0) > 0 and w[w.index(0) - 1] in BAD


@pytest.mark.parametrize("beam_size,G", FK.SHAPES)
def test_a_plain_search_of_the_stand_in_repeats_trigrams(beam_size, G):
    least, of = PLAIN_REPEATS[(beam_size, G)]
    for salt in SALTS:
        (_, _, done), rules = run(beam_size, G, salt)
        assert not rules.active and all("rule_stats" not in b for _, b, _ in kept(done))
        ws = [w for _, _, w in kept(done)]
        assert len(ws) == of
        assert sum(FK.repeats_trigram(w, FK.length_of(w, T)) for w in ws) >= least


@pytest.mark.parametrize("beam_size,G", FK.SHAPES)
def test_a_hard_block_leaves_no_repeated_trigram_in_any_kept_beam(beam_size, G):
    fired = 0
    for salt in SALTS:
        (seq, seqlp, done), rules = run(beam_size, G, salt, block_trigrams=1, trigram_alpha=math.inf)
        assert rules.flags == 1 and np.isneginf(rules.trigram_pen)
        for s, b, w in kept(done):
            L = FK.length_of(w, T)
            assert not FK.repeats_trigram(w, L), (salt, s, w)
            np.testing.assert_array_equal(b["rule_stats"], sequence_events(w, L, rules))
            fired += int(b["rule_stats"][0])
        for s in range(N_SUB):
            assert seq[s].equal(done[s][0]["seq"]) and seqlp[s].equal(done[s][0]["logps"])
    assert fired > 0                                                             # the penalty did act: the beams were pushed off the cycle


@pytest.mark.parametrize("beam_size,G", FK.SHAPES)
def test_no_kept_beam_ends_behind_a_listed_word(beam_size, G):
    plain_bad = ruled_events = 0
    for salt in SALTS:
        (_, _, done), _ = run(beam_size, G, salt, end_boost=4.0)
        plain_bad += sum(ends_badly(w) for _, _, w in kept(done))
        (_, _, done), rules = run(beam_size, G, salt, end_boost=4.0, block_bad_endings=1, bad_ending_ids=list(BAD))
        assert rules.flags == 8 and rules.bad_ids == BAD
        for s, b, w in kept(done):
            assert not ends_badly(w), (salt, s, w)                               # (a beam cut at T has no end token at all)
            ruled_events += int(b["rule_stats"][2])
            assert b["rule_stats"][1] == 0 and b["rule_stats"][3] == -1
    assert plain_bad > 0 and ruled_events > 0


@pytest.mark.parametrize("beam_size,G", FK.SHAPES)
def test_every_log_prob_is_the_ruled_value_on_the_beams_own_prefix(beam_size, G):
    moved = 0
    for salt in SALTS:
        (_, _, done), rules = run(beam_size, G, salt, block_trigrams=1, trigram_alpha=2.0, block_bad_endings=1, bad_ending_ids=list(BAD))
        assert rules.trigram_pen == np.float32(np.float32(-0.693) * np.float32(2.0))
        tab = FK.table(N_SUB, salt)
        plain = DecodeRules()
        for s, b, w in kept(done):
            L = FK.length_of(w, T)
            lp = b["logps"].numpy()
            for t in range(L):
                want = FK.ruled_row(tab, s, w, t, rules)[w[t]]
                if w[t] == FK.V1 - 1:
                    want = np.float32(want - np.float32(1000))                  # the beam step's own UNK penalty, on the ruled value
                assert lp[t] == want, (salt, s, w, t)
                moved += want != FK.ruled_row(tab, s, w, t, plain)[w[t]]
            assert not lp[L:].any()
            assert b["unaug_p"] == float(lp.sum(dtype=np.float32))
    assert moved > 0                                                             # some chosen word did carry a penalty


def test_sequence_events_on_hand_worked_rows():
    tri = DecodeRules(block_trigrams=1)
    both = DecodeRules(block_trigrams=1, block_bad_endings=1, bad_ids=(2, 7))
    #        step:  0  1  2  3  4  5  6  7
    row = [1, 2, 3, 1, 2, 3, 1, 0]
    # a penalty applies at step t when (h[t-2], h[t-1]) occurred earlier: t = 5 (1 2 | 1 2), 6 (2 3 | 2 3), 7 (3 1 | 3 1)
    np.testing.assert_array_equal(sequence_events(row, 8, tri), [3, 0, 0, -1])
    np.testing.assert_array_equal(sequence_events(row, 6, tri), [1, 0, 0, -1])
    np.testing.assert_array_equal(sequence_events(row, 5, tri), [0, 0, 0, -1])
    # the bad-ending ban applies at step t when h[t-1] is listed: after the 2s at steps 2 and 5
    np.testing.assert_array_equal(sequence_events(row, 8, both), [3, 0, 2, -1])
    np.testing.assert_array_equal(sequence_events(row, 2, both), [0, 0, 0, -1])
    np.testing.assert_array_equal(sequence_events([7, 7, 7, 7, 7], 5, both), [2, 0, 4, -1])    # (7 7 | 7 7) at steps 3 and 4
    np.testing.assert_array_equal(sequence_events([5, 0, 0, 0], 1, both), [0, 0, 0, -1])
    assert sequence_events(row, 8, tri).dtype == np.int32
    np.testing.assert_array_equal(sequence_events(row, 8, DecodeRules()), [0, 0, 0, -1])


def test_sequence_events_are_the_restatements_events_summed_over_steps():
    rng = np.random.default_rng(5)
    rules = DecodeRules(block_trigrams=1, block_bad_endings=1, bad_ids=(1, 3))
    for _ in range(40):
        L = int(rng.integers(1, 13))
        row = rng.integers(0, 4, size=12)
        ev = np.zeros(4, np.int64)
        for t in range(L):
            ev += apply_rules_restatement(rng.normal(size=9), row, t, rules, return_events=True)[1][0]
        got = sequence_events(row, L, rules)
        assert got[0] == ev[0] and got[2] == ev[2] and got[1] == 0 and got[3] == -1


@pytest.mark.parametrize("g", [1, 2])
def test_a_minus_one_prefix_changes_nothing_for_a_live_beam(g):
    """The device keeps word w of group g in column g + w behind g columns of -1 and passes ONE step number for every group.  A live
    beam has t >= 1 words; a match of block_trigrams needs h[j + 1] == h[last] >= 0 and h[j] == h[last - 1], which is >= 0 whenever it
    is consulted with two or more words and which no j inside the prefix can pair with a real successor otherwise; the bad-ending ban
    reads h[last] only."""
    rules = DecodeRules(block_trigrams=1, trigram_alpha=2.0, block_bad_endings=1, bad_ids=(0, 2))
    hard = DecodeRules(block_trigrams=1, trigram_alpha=math.inf, block_bad_endings=1, bad_ids=(1,))
    x = np.random.default_rng(9).integers(-8, 9, size=11) / 4
    hits = 0
    for t in range(1, 7):
        for h in itertools.product(range(3), repeat=t):
            for r in (rules, hard):
                want, ev = apply_rules_restatement(x, list(h), t, r, return_events=True)
                got, ev2 = apply_rules_restatement(x, [-1] * g + list(h), t + g, r, return_events=True)
                assert np.array_equal(got.view(np.int64), want.view(np.int64)) and np.array_equal(ev, ev2), (h, g)
                hits += int(ev[0, 0])
    assert hits > 0
    # t = 0 (the <bos> step, and a group that has not started): nothing fires on an all -1 history either
    for t0 in range(0, g + 3):
        got, ev = apply_rules_restatement(x, [-1] * t0, t0, rules, return_events=True)
        assert np.array_equal(got, apply_rules_restatement(x, [], 0, rules)) and not ev[0, :3].any()


def test_shifted_history_layout():
    words = np.array([[5, 6, 7, 9], [1, 2, -1, -1], [3, 3, 3, 3]])
    out = beam.shifted_history(words, [3, 2, 0], 3, 6)
    np.testing.assert_array_equal(out, [[5, 6, 7, -1, -1, -1], [-1, 1, 2, -1, -1, -1], [-1] * 6])
    with pytest.raises(ValueError, match="holds 3 words before step 2"):
        beam.shifted_history(words, [3, 2, 0], 2, 6)


def test_from_beam_options_defaults_key_and_refusals():
    assert not DecodeRules.from_beam_options({}).active and DecodeRules.from_beam_options(None).key is None
    assert not DecodeRules.from_beam_options({"beam_size": 2}).active
    assert not DecodeRules.from_beam_options({"beam_size": 2, "beam_rules": {}}).active
    r = DecodeRules.from_beam_options({"beam_size": 2, "beam_rules": {"block_trigrams": 1}})
    assert r.active and r.flags == 1 and r.trigram_alpha == 2.0 and r.bad_ids == () and not r.decoding_constraint and not r.suppress_unk
    assert r.key == (1, float(np.float32(np.float32(-0.693) * np.float32(2.0))), ())
    hash(r.key)
    r = DecodeRules.from_beam_options({"beam_size": 3, "beam_rules": {"block_trigrams": 1, "trigram_alpha": math.inf, "block_bad_endings": 1,
                                                                     "bad_ending_ids": [4, 2]}})
    assert r.flags == 9 and r.key == (9, -math.inf, (4, 2))
    r = DecodeRules.from_beam_options({"beam_size": 2, "beam_rules": {"block_bad_endings": 1}}, ix_to_word={"3": "the", "5": "dog", "9": "with"})
    assert r.flags == 8 and r.bad_ids == (3, 9)
    # the top-level decoding_constraint keeps its beam meaning beside the key
    assert DecodeRules.from_beam_options({"beam_size": 2, "decoding_constraint": 1, "beam_rules": {"block_trigrams": 1}}).flags == 1
    for size in (1, 0, None):
        o = {"beam_rules": {"block_trigrams": 1}}
        if size is not None:
            o["beam_size"] = size
        with pytest.raises(ValueError, match="beam_rules with beam_size = .*top-level keys block_trigrams, trigram_alpha, block_bad_endings"):
            DecodeRules.from_beam_options(o)
    for name in ("decoding_constraint", "suppress_unk"):
        with pytest.raises(ValueError, match=rf"beam_rules\['{name}'\]: beam search has its own repeat ban"):
            DecodeRules.from_beam_options({"beam_size": 2, "beam_rules": {name: 1}})
    with pytest.raises(ValueError, match=r"unknown key\(s\) \['block_trigram'\]"):
        DecodeRules.from_beam_options({"beam_size": 2, "beam_rules": {"block_trigram": 1}})
    with pytest.raises(ValueError, match="must be a dict"):
        DecodeRules.from_beam_options({"beam_size": 2, "beam_rules": 1})
    with pytest.raises(ValueError, match="block_bad_endings needs the ids"):
        DecodeRules.from_beam_options({"beam_size": 2, "beam_rules": {"block_bad_endings": 1}})
    with pytest.raises(ValueError, match="bad_ids holds 65 ids: the bad-ending list takes at most 64"):
        DecodeRules.from_beam_options({"beam_size": 2, "beam_rules": {"block_bad_endings": 1, "bad_ending_ids": list(range(65))}})
    for alpha in (-1.0, math.nan):
        with pytest.raises(ValueError, match="the trigram penalty needs alpha >= 0"):
            DecodeRules.from_beam_options({"beam_size": 2, "beam_rules": {"block_trigrams": 1, "trigram_alpha": alpha}})


def test_the_top_level_refusals_are_unchanged():
    for name in ("block_trigrams", "block_bad_endings", "suppress_unk"):
        with pytest.raises(ValueError, match=f"^{name} = 1 with beam_size = 2: the decode rules act on the greedy / sampling loop only"):
            DecodeRules.from_options({"beam_size": 2, name: 1})
    assert not DecodeRules.from_options({"decoding_constraint": 1, "beam_size": 3}).active
    assert not DecodeRules.from_options({"beam_size": 2, "beam_rules": {"block_trigrams": 1}}).active      # the new key is not a top-level rule
    assert DecodeRules.from_options({"block_trigrams": 1}).flags == 1


def test_history_wider_than_the_rules_kernel_takes_is_refused():
    o = opt_of(4, 2, block_trigrams=1)
    with pytest.raises(ValueError, match="T \\+ group_size - 1 = 65 columns; the limit is 64"):
        beam.search(FK.HostEngine(1, 4, (3,), N, 0), 64, o, rules=DecodeRules.from_beam_options(o))
    beam.check_rule_limits(64, 1)


def test_an_engine_that_cannot_rule_its_rows_refuses():
    eng = beam._StepEngine.__new__(beam._StepEngine)
    hist = beam.RuleHistory(DecodeRules(block_trigrams=1), np.zeros((1, 4), np.int64), np.zeros(1, np.int64), 0, 4)
    for call in (lambda: eng.first(3, history=hist), lambda: eng.advance(np.zeros(1, np.int64), 3, history=hist)):
        with pytest.raises(ValueError, match="beam_rules: the step-API engine"):
            call()
