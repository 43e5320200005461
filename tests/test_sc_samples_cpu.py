"""The one-pass self-critical step (sc_samples >= 2) without a GPU: the leave-one-out reward contract of
`SelfCriticalReward.enqueue_loo` as `loo_reward_restatement` restates it, fixture (a) of tests/golden/make_golden_sc_samples.py, the option's
handling, and that the feature adds no entry point (the header table stays at 14 headers / 172 names).

The error bound.  Every operation of the contract is one correctly rounded fp64 operation (relative error <= eps = 2^-53).  With
A = sum_k |s_k| over a caption row's samples: the n - 1 adds of `tot` err by at most (n - 1) eps A; `tot - s_k` adds eps |rest|; the
division by n - 1 brings both down to eps A + eps |b| and adds eps |b|; the last subtraction adds eps |r|.  |b| <= A / (n - 1) and
|r| <= |s_k| + |b|, so for n = 2 the sum is at most eps A (1 + 2 + 1) and for n >= 3 at most eps A (1 + 1 + 1.5): 4 eps A either way,
which is the "4 * 2^-53 relative" of the contract, relative to A.  A group's n rewards sum to 0 exactly in exact arithmetic, so their
exact sum is within n such bounds of 0."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import sc_samples_golden as SG
from subgc import _lib, selfcritical
import subgc.models as models

EPS = SG.EPS


def groups(n, b5, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "scores":                                   # what a reward looks like: CIDEr + BLEU of a few tenths, some zeros
        s = rng.random((n, b5)) * rng.choice([0.0, 0.3, 2.5], (n, b5))
    elif kind == "signed":
        s = rng.standard_normal((n, b5)) * 10.0 ** rng.integers(-3, 4, (n, b5))
    else:                                                  # one sample dwarfs the others
        s = rng.random((n, b5)) * 1e-9
        s[rng.integers(0, n, b5), np.arange(b5)] = 7.0
    return s.reshape(-1)


@pytest.mark.parametrize("kind", ["scores", "signed", "spread"])
@pytest.mark.parametrize("n", [2, 3, 5, 16])
def test_restatement_is_the_mean_of_the_others_within_four_roundings(n, kind):
    b5 = 7
    s = groups(n, b5, kind, 100 * n + len(kind))
    reward, baseline, mean = selfcritical.loo_reward_restatement(s, n)
    assert reward.dtype == np.float32 and baseline.dtype == np.float64 and reward.shape == baseline.shape == (n * b5,)
    r64 = s - baseline                                                       # the contract's last fp64 operation, before the cast
    assert np.array_equal(reward, r64.astype(np.float32))
    want_r, want_b = SG.loo_fraction(s, n)
    A = np.abs(s.reshape(n, b5)).sum(0)
    worst = 0.0
    for c in range(b5):
        bound = Fraction(4) * Fraction(EPS) * Fraction(float(A[c]))
        total = Fraction(0)
        for k in range(n):
            r = k * b5 + c
            err = abs(Fraction(float(r64[r])) - want_r[r])
            assert err <= bound and abs(Fraction(float(baseline[r])) - want_b[r]) <= bound, (n, kind, c, k)
            worst = max(worst, float(err / bound)) if bound else worst
            total += Fraction(float(r64[r]))
        assert abs(total) <= n * bound, (n, kind, c)                         # the group's rewards sum to 0
    assert mean == float(reward.astype(np.float64).mean())
    print(f"n={n} {kind}: worst error / bound {worst:.3f}")


def test_two_samples_are_the_exact_pairwise_difference():
    """n = 2: baseline_0 = (s_0 + s_1) - s_0.  Where the sum is exact -- scores on a common grid of 2^-30 below 2^20, as here -- this is
    s_1 itself and the reward is float32(s_0 - s_1) bit for bit, the reward subgc_sc_reward forms.  For arbitrary doubles the sum's
    rounding (<= eps (s_0 + s_1)) can move the fp32 result only where s_0 - s_1 lies that close to a rounding boundary of fp32."""
    rng = np.random.default_rng(5)
    b5 = 64
    s = rng.integers(0, 2 ** 50, (2, b5)).astype(np.float64) * 2.0 ** -30
    s[0, 0], s[1, 0] = 0.0, 0.0
    s[0, 1] = s[1, 1]
    reward, baseline, _ = selfcritical.loo_reward_restatement(s.reshape(-1), 2)
    assert np.array_equal(baseline.reshape(2, b5), s[::-1])
    assert np.array_equal(reward.reshape(2, b5)[0], (s[0] - s[1]).astype(np.float32))
    assert np.array_equal(reward.reshape(2, b5)[1], (s[1] - s[0]).astype(np.float32))
    assert np.array_equal(reward.reshape(2, b5)[0], -reward.reshape(2, b5)[1])
    # arbitrary doubles: within one fp32 rounding of the pairwise difference, and the error before the cast obeys the bound
    s = groups(2, 500, "scores", 9).reshape(2, -1)
    reward, baseline, _ = selfcritical.loo_reward_restatement(s.reshape(-1), 2)
    assert (np.abs(baseline.reshape(2, -1) - s[::-1]) <= EPS * (s[0] + s[1]) + EPS * s[::-1]).all()      # the add's rounding, then the subtract's
    d32 = (s[0] - s[1]).astype(np.float32)
    same = reward.reshape(2, -1)[0] == d32
    print(f"n=2 on arbitrary doubles: {int(same.sum())} of {same.size} rewards are the pairwise difference bit for bit")
    assert (np.abs(reward.reshape(2, -1)[0] - d32) <= np.spacing(np.abs(d32))).all()


@pytest.mark.parametrize("n", [2, 3, 5, 16])
def test_equal_samples_give_reward_zero_exactly(n):
    """Equal scores on a grid of 2^-40 below 1: n s is exact for n <= 16 (four more bits), so tot - s = (n - 1) s and the division
    gives s back."""
    rng = np.random.default_rng(n)
    one = rng.integers(0, 2 ** 40, 9).astype(np.float64) * 2.0 ** -40
    s = np.tile(one, n)
    reward, baseline, mean = selfcritical.loo_reward_restatement(s, n)
    assert not reward.any() and np.array_equal(baseline, s) and mean == 0.0


def test_restatement_refuses_one_sample():
    with pytest.raises(ValueError, match="n = 1"):
        selfcritical.loo_reward_restatement(np.zeros(4), 1)


@pytest.mark.parametrize("n", SG.NS_CASE)
def test_fixture_rewards_are_the_restatements_bit_for_bit(n):
    z = SG.load("sc_samples_case.npz")
    wc, wb = z["weights"]
    scores = wc * z[f"n{n}.cider"] + wb * z[f"n{n}.bleu"][:, 3]
    assert np.array_equal(scores, z[f"n{n}.scores"])
    reward, baseline, mean = selfcritical.loo_reward_restatement(scores, n)
    assert np.array_equal(reward, z[f"n{n}.reward"]) and reward.dtype == z[f"n{n}.reward"].dtype
    assert np.array_equal(baseline, z[f"n{n}.baseline"]) and mean == float(z[f"n{n}.mean_reward"])
    tok = z[f"n{n}.tok"]
    rows = tok.shape[0] // n
    assert not tok[0].any() and tok[rows + 1].all() and np.array_equal(tok[(n - 1) * rows + 2], tok[2])      # the rows the fixture promises
    k = (n - 1) * rows + 2
    assert scores[k] == scores[2]                                                # identical samples score alike ...
    if n == 2:
        assert reward[2] == 0.0 and reward[k] == 0.0                             # ... and with nobody else in the group, earn nothing
    # the reference's RewardCriterion on the stored log-probabilities: restated in fp64 (misc/utils.py:89-109)
    seq = np.concatenate([tok, np.zeros((tok.shape[0], 1), np.int64)], 1)
    m = np.ones(seq.shape)
    m[:, 1:] = seq[:, :-1] > 0
    want = float((-z[f"n{n}.logp"].astype(np.float64) * reward[:, None].astype(np.float64) * m).sum() / m.sum())
    assert abs(want - float(z[f"n{n}.loss"])) <= 16 * 2.0 ** -24 * np.abs(z[f"n{n}.logp"] * reward[:, None] * m).sum() / m.sum()


def test_train_fixture_holds_every_case_and_stays_below_the_file_limit():
    path = os.path.join(SG.GOLDEN, "sc_samples_train.npz")
    assert os.path.getsize(path) < 1 << 20
    z = SG.load("sc_samples_train.npz")
    for name in SG.MODELS:
        for n in SG.NS_TRAIN:
            pre = f"{name}.n{n}."
            tok = z[pre + "sc.tok"]
            b5 = tok.shape[0] // n
            assert tok.shape[0] == n * b5 and not tok[4].any() and tok[b5 + 6].all() and np.array_equal(tok[(n - 1) * b5 + 9], tok[9])
            reward, baseline, mean = selfcritical.loo_reward_restatement(z[pre + "sc.scores"], n)
            assert np.array_equal(reward, z[pre + "sc.reward"]) and np.array_equal(baseline, z[pre + "sc.baseline"])
            assert any(k.startswith(pre + "grad.logit.weight") for k in z) and np.isfinite(z[pre + "lang_loss"])


# ----------------------------------------------------------------------------------------------------------------- the option
class _Opt:
    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.mark.parametrize("bad", [0, -1, 17, 2.5, 2.0])
def test_option_refuses_what_is_no_sample_count_with_the_number(bad):
    for kw, opt in (({"sc_samples": bad}, None), ({}, _Opt(train_sample_n=bad))):
        with pytest.raises(ValueError, match=re.escape(repr(bad))):
            models.LossWrapper(None, opt, **kw)


def test_option_one_and_absent_select_the_existing_path():
    assert models.LossWrapper(None, None).sc_samples == 1
    assert models.LossWrapper(None, _Opt()).sc_samples == 1
    assert models.LossWrapper(None, None, sc_samples=1).sc_samples == 1
    assert models.LossWrapper(None, _Opt(train_sample_n=1)).sc_samples == 1
    assert models.LossWrapper(None, _Opt(train_sample_n=5)).sc_samples == 5
    assert models.LossWrapper(None, _Opt(train_sample_n=5), sc_samples=2).sc_samples == 2      # the argument wins
    assert models.LossWrapper(None, None, sc_samples=16).sc_samples == 16


# ----------------------------------------------------------------------------------------------------------------- no new entry point
def test_header_table_still_has_14_rows_and_172_names():
    inc = os.path.dirname(_lib.HEADER)
    names = [n for hdr in _lib.HEADERS.values() for n in _lib.parse_header(os.path.join(inc, hdr))]
    assert len(_lib.HEADERS) == 14 and len(names) == len(set(names)) == 172


def test_selfcritical_module_names_only_declared_entry_points():
    inc = os.path.dirname(_lib.HEADER)
    declared = {n for hdr in _lib.HEADERS.values() for n in _lib.parse_header(os.path.join(inc, hdr))}
    with open(selfcritical.__file__) as f:
        named = set(re.findall(r"\bsubgc_[a-z0-9_]+\b", f.read()))
    named -= {"subgc_selfcritical_hip"}                                          # the header's own file name
    assert named and not named - declared, sorted(named - declared)
