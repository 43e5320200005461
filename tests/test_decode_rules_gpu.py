"""The decode-rules kernel (include/subgc_decode_rules_hip.h) against the numpy restatement of its contract
(subgc.decode_rules.apply_rules_restatement): the set of altered columns, every -inf position and every counter equal, finite values
within the bound DESIGN 4.W derives (coded once, in decode_rules_reference.ruled_bound); equal logits give equal bits; the three pick
paths on a ruled row; prev_count == 0; every refusal with its number."""
import numpy as np
import pytest
import torch

import decode_rules_reference as R
from subgc import _lib, ops
from subgc._lib import SubgcError
from subgc.decode_rules import DecodeRules, apply_rules_restatement

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VS = [8, 37, 256, 257, 1001, 9488]
NS = [1, 3, 37]
TS = [4, 20, 64]


def _steps(T):
    return sorted({0, 1, 2, 3, min(4, T - 1), T - 1})


def _logits(n, V, ld_extra, seed, quarter=False):
    g = torch.Generator().manual_seed(seed)
    if quarter:
        x = torch.randint(-8, 9, (n, V + ld_extra), generator=g).float() / 4
    else:
        x = torch.randn(n, V + ld_extra, generator=g) * 4
    return x.to(DEV)[:, :V]


def _rules(V, **kw):
    return DecodeRules(bad_ids=R.bad_ids_for(V), **kw)


def _run(x, h, t, rules, stats=True, prev=None, flags=None):
    """-> (ruled rows fp32 [n, V] on the host, stats [n, 4] or None); x is left alone (the kernel works on a copy of the same pitch)."""
    n, V = x.shape
    buf = torch.empty(n, x.stride(0), device=DEV)
    row = buf[:, :V]
    row.copy_(x)
    if buf.size(1) > V:
        buf[:, V:] = 77.0                                                       # the padding between rows is never touched
    seq = torch.from_numpy(np.ascontiguousarray(h)).to(DEV)
    st = torch.zeros(n, 4, device=DEV, dtype=torch.int32) if stats else None
    bad = torch.tensor(rules.bad_ids, device=DEV, dtype=torch.int32) if rules.block_bad_endings else None
    pc = None if prev is None else torch.tensor([prev], device=DEV, dtype=torch.int32)
    ops.decode_rules(row, seq, t, rules.flags if flags is None else flags, rules.trigram_pen, bad, st, pc)
    torch.cuda.synchronize()
    if buf.size(1) > V:
        assert (buf[:, V:] == 77.0).all()
    return row.cpu().numpy().copy(), None if st is None else st.cpu().numpy()


def _check(x, h, t, rules, plain_dev, what):
    """One launch against the restatement.  plain_dev: the device's own log-softmax of x (the launch with no flag), whose bits every
    untouched column must keep.  -> the worst |error| / bound met."""
    got, stats = _run(x, h, t, rules)
    x64 = x.double().cpu().numpy()
    want, ev = apply_rules_restatement(x64, h, t, rules, return_events=True)
    plain = apply_rules_restatement(x64, h, t, DecodeRules())
    assert not np.isnan(got).any(), what
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(want), err_msg=what)
    np.testing.assert_array_equal(got.view(np.int32) != plain_dev.view(np.int32), want != plain, err_msg=what + ": altered columns")
    np.testing.assert_array_equal(stats, ev, err_msg=what + ": stats")
    worst = 0.0
    for r in range(x.size(0)):
        b = R.ruled_bound(x64[r], h[r], t, rules)
        fin = np.isfinite(want[r])
        err = np.abs(got[r][fin].astype(np.float64) - want[r][fin])
        assert (err <= b[fin]).all(), (what, r, float((err / b[fin]).max()))
        worst = max(worst, float((err / b[fin]).max()))
    return worst


@pytest.mark.parametrize("ld_extra", [0, 3])
@pytest.mark.parametrize("V", VS)
def test_kernel_equals_the_restatement(V, ld_extra):
    worst, launches, seen3 = 0.0, 0, False
    for n in NS:
        x = _logits(n, V, ld_extra, 1000 + V + n)
        x64 = x.double().cpu().numpy()
        for T in TS:
            for t in _steps(T):
                h = R.histories(n, T, t, V, first=(t + T) % 6)
                plain_dev, _ = _run(x, h, t, DecodeRules(), stats=False, flags=0)
                pl = apply_rules_restatement(x64, h, t, DecodeRules())
                for r in range(n):
                    b = R.ruled_bound(x64[r], h[r], t, DecodeRules())
                    assert (np.abs(plain_dev[r] - pl[r]) <= b).all()
                # every rule alone and all together on the widest batch; all together and the trigram rule alone on the others
                sets = R.EACH_AND_ALL if n == NS[-1] else (R.EACH_AND_ALL[0], R.EACH_AND_ALL[-1])
                for kw in sets:
                    worst = max(worst, _check(x, h, t, _rules(V, **kw), plain_dev, f"V={V} n={n} T={T} t={t} {sorted(kw)}"))
                    launches += 1
                seen3 = seen3 or any(max(R.trigram_counts(h[r], t, V).values(), default=0) >= 3 for r in range(n))
    assert seen3                                                                # a multiplicity of three or more was among the cases
    print(f"V = {V}, ld = V + {ld_extra}: {launches} launches, worst |ruled - restatement| / bound = {worst:.3f}")


@pytest.mark.parametrize("V", VS)
def test_a_hard_block_writes_minus_infinity_on_counted_columns_only(V):
    n, T, t = 6, 20, 19
    x = _logits(n, V, 3, 5 + V)
    h = R.histories(n, T, t, V)
    rules = _rules(V, block_trigrams=1, trigram_alpha=float("inf"))
    plain_dev, _ = _run(x, h, t, DecodeRules(), stats=False, flags=0)
    _check(x, h, t, rules, plain_dev, f"V={V} alpha=inf")
    got, _ = _run(x, h, t, rules)
    cols = [sorted(R.trigram_counts(h[r], t, V)) for r in range(n)]
    assert [np.flatnonzero(np.isneginf(got[r])).tolist() for r in range(n)] == cols and any(cols)


@pytest.mark.parametrize("V", VS)
def test_equal_logits_give_equal_bits_and_the_ruled_first_argmax_is_the_restatements(V):
    n, T = 37, 20
    x = _logits(n, V, 3, 77 + V, quarter=True)
    x64 = x.double().cpu().numpy()
    xh = x.cpu().numpy()
    for t in (0, 4, 19):
        h = R.histories(n, T, t, V, first=t)
        rules = _rules(V, **R.EACH_AND_ALL[-1])
        plain_dev, _ = _run(x, h, t, DecodeRules(), stats=False, flags=0)
        got, stats = _run(x, h, t, rules)
        want, ev = apply_rules_restatement(x64, h, t, rules, return_events=True)
        for r in range(n):
            for v in np.unique(xh[r]):
                assert np.unique(plain_dev[r][xh[r] == v].view(np.int32)).size == 1
            same = got[r].view(np.int32) == plain_dev[r].view(np.int32)
            assert same.sum() >= V - 5
            assert int(np.argmax(got[r])) == int(np.argmax(want[r])), (V, t, r)
        np.testing.assert_array_equal(stats, ev)
        again, _ = _run(x, h, t, rules)
        np.testing.assert_array_equal(again.view(np.int32), got.view(np.int32))  # the same launch twice: the same bits


def _pick(row_dev, k, top_p, u, t, seq0):
    n = row_dev.size(0)
    seq = seq0.clone()
    seqlp = torch.zeros(seq.shape, device=DEV)
    it, unf = torch.zeros(n, device=DEV, dtype=torch.int64), torch.ones(n, device=DEV, dtype=torch.int32)
    flag = torch.zeros(1, device=DEV, dtype=torch.int32)
    ops.decode_pick(row_dev, k, 0.6, u, t, seq, seqlp, it, unf, flag, None, raw=False, top_p=top_p)
    torch.cuda.synchronize()
    return seq[:, t].cpu().numpy(), seqlp[:, t].cpu().numpy()


@pytest.mark.parametrize("V", VS)
def test_a_ruled_row_through_the_three_pick_paths(V):
    """greedy, k = 3 (subgc_decode_pick) and k = 20 with the_p = 0.9 (subgc_decode_sample; k = V where the row has fewer columns) on
    the device's ruled row and on the restatement's row uploaded as fp32: the same tokens, and never a -inf column."""
    n, T, t = 37, 20, 19
    x = _logits(n, V, 3, 300 + V)
    h = R.histories(n, T, t, V)
    h[:, :t] = np.where(h[:, :t] == 0, 1, h[:, :t])                            # live rows: `unfinished` is all ones below
    rules = _rules(V, **R.EACH_AND_ALL[-1])
    got, _ = _run(x, h, t, rules)
    want = apply_rules_restatement(x.double().cpu().numpy(), h, t, rules)
    banned = np.isneginf(want)
    assert banned.any(1).all()
    dev_row, ref_row = torch.from_numpy(got).to(DEV), torch.from_numpy(want.astype(np.float32)).to(DEV)
    seq0 = torch.from_numpy(h).to(DEV)
    g = torch.Generator().manual_seed(V)
    u = torch.rand(n, generator=g).to(DEV)
    for k, top_p in ((0, 1.0), (3, 1.0), (min(20, V), 0.9)):
        a, alp = _pick(dev_row, k, top_p, u if k else None, t, seq0)
        b, blp = _pick(ref_row, k, top_p, u if k else None, t, seq0)
        np.testing.assert_array_equal(a, b, err_msg=f"V={V} k={k}")
        assert not banned[np.arange(n), a].any() and np.isfinite(alp).all()
        assert np.abs(alp - blp).max() <= 1e-4
        if k == 0:
            np.testing.assert_array_equal(a, want.argmax(1))
            np.testing.assert_array_equal(alp.view(np.int32), got[np.arange(n), a].view(np.int32))      # greedy reports the ruled value


def test_prev_count_zero_writes_nothing():
    V, n, T, t = 257, 3, 20, 5
    x = _logits(n, V, 3, 9)
    h = R.histories(n, T, t, V)
    rules = _rules(V, **R.EACH_AND_ALL[-1])
    got, stats = _run(x, h, t, rules, prev=0)
    np.testing.assert_array_equal(got.view(np.int32), x.cpu().numpy().view(np.int32))
    assert not stats.any()
    on, stats_on = _run(x, h, t, rules, prev=1)
    ref, stats_ref = _run(x, h, t, rules)
    np.testing.assert_array_equal(on.view(np.int32), ref.view(np.int32))
    np.testing.assert_array_equal(stats_on, stats_ref)
    assert stats_ref.any()
    # the counters accumulate: a second step on top of the first
    seq = torch.from_numpy(h).to(DEV)
    st = torch.from_numpy(stats_ref.astype(np.int32)).to(DEV)
    ops.decode_rules(x.clone(), seq, t, rules.flags, rules.trigram_pen, torch.tensor(rules.bad_ids, device=DEV, dtype=torch.int32), st)
    np.testing.assert_array_equal(st.cpu().numpy(), 2 * stats_ref)
    # without counters the rows are the same
    bare, none = _run(x, h, t, rules, stats=False)
    np.testing.assert_array_equal(bare.view(np.int32), ref.view(np.int32))
    assert none is None


def test_every_refusal_names_its_number():
    V, n, T = 64, 2, 8
    x = torch.zeros(n, V, device=DEV)
    seq = torch.zeros(n, T, device=DEV, dtype=torch.int64)
    bad = torch.zeros(80, device=DEV, dtype=torch.int32)
    P = lambda t_: t_.data_ptr()

    def call(**kw):
        a = dict(logits=P(x), ld=V, n=n, V=V, seq=P(seq), T=T, t=3, flags=15, pen=-1.386, bad=P(bad), n_bad=4, stats=None, prev=None)
        a.update(kw)
        _lib.call_decode_rules("subgc_decode_rules", a["logits"], a["ld"], a["n"], a["V"], a["seq"], a["T"], a["t"], a["flags"], a["pen"],
                               a["bad"], a["n_bad"], a["stats"], a["prev"], None)

    call()
    torch.cuda.synchronize()
    for kw, msg in ((dict(V=16385, ld=16385), "V = 16385"), (dict(V=7), "V = 7"), (dict(T=65), "T = 65"), (dict(t=8), "t = 8"),
                    (dict(t=-1), "t = -1"), (dict(n_bad=65), "n_bad = 65"), (dict(ld=63), "ld = 63"), (dict(flags=16), "flags = 16"),
                    (dict(flags=-1), "flags = -1"), (dict(n=-2), "n = -2")):
        with pytest.raises(SubgcError, match="decode_rules: .*" + msg):
            call(**kw)
    call(n=0, logits=None, seq=None)                                             # no rows: nothing to do
    with pytest.raises(SubgcError, match="null pointer"):
        call(logits=None)
    with pytest.raises(SubgcError, match="n_bad = 4 ids but bad_ids is null"):
        call(bad=None)
    with pytest.raises(SubgcError, match="stats must be a contiguous"):
        ops.decode_rules(x, seq, 1, 1, -1.386, stats=torch.zeros(n, 3, device=DEV, dtype=torch.int32))
    with pytest.raises(SubgcError, match="seq must be a contiguous"):
        ops.decode_rules(x, seq[:1], 1, 1, -1.386)
    torch.cuda.synchronize()


def test_debug_bounds_reports_a_history_token_outside_the_row_and_the_kernel_ignores_it():
    V, n, T, t = 37, 2, 8, 5
    x = _logits(n, V, 0, 3)
    h = np.array([[1, 2, V + 4, 1, 2, 0, 0, 0], [3, -2, -2, -2, -2, 0, 0, 0]], np.int64)
    rules = _rules(V, **R.EACH_AND_ALL[-1])
    got, stats = _run(x, h, t, rules)                                          # row 0: the counted column is out of range; row 1: the last word is
    want, ev = apply_rules_restatement(x.double().cpu().numpy(), h, t, rules, return_events=True)
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(want))
    np.testing.assert_array_equal(stats, ev)
    assert stats[:, 0].tolist() == [0, 0] and stats[1, 1] == 0 and np.abs(got[np.isfinite(want)] - want[np.isfinite(want)]).max() < 1e-3
    with ops.debug_bounds():
        with pytest.raises(SubgcError, match="decode_rules: seq"):
            _run(x, h, t, rules)
        _run(x, h, 1, rules)                                                   # the first column is in range
