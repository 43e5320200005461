"""The row rules of csrc/rowwise.h and csrc/criterion_rule.h as the entry points that share them expose them: the same small hand-made
rows go through every entry point that holds one rule, and the outputs must agree -- to the bit wherever the kernels perform the same
operations in the same order.
  (a) the row log-sum-exp: row_lse, row_lse_sum and log_softmax_rows_;
  (b) the greedy choice and the filing of its token: decode_pick(k = 0), sc_pick(n_sample = 0) and forced_pick given that token;
  (c) the criterion fused through the log-softmax: the plain rule against the smoothed rule with smoothing = 0 (conf = 1, e = 0, H = 0:
      the extra terms are exact zeros), and the rows all three backwards must zero."""
import numpy as np
import pytest
import torch

from subgc import forced, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDTHS = [1, 37, 256, 257, 1024, 1025, 4096, 4097, 10240, 10241, 16384]        # the edges of the PER ladder (4 / 16 / 40 / 64 x 256)
T_SEQ = 3


def rows_for(V):
    """Five rows of width V: constant, a +50 offset, a one-hot spike in the last column, two equal maxima at columns 255 and 256 (the
    first arg-max across the thread boundary; clipped to the last column of a narrower row), seeded normal."""
    rng = np.random.RandomState(1000 + V)
    x = np.empty((5, V), np.float32)
    x[0] = 0.5
    x[1] = rng.randn(V).astype(np.float32) + np.float32(50.0)
    x[2] = 0.0
    x[2, V - 1] = 20.0
    x[3] = 0.1 * rng.randn(V).astype(np.float32)
    x[3, min(255, V - 1)] = 5.0
    x[3, min(256, V - 1)] = 5.0
    x[4] = rng.randn(V).astype(np.float32)
    return torch.from_numpy(x).to(DEV)


# ---------------------------------------------------------------- (a)
@pytest.mark.parametrize("V", WIDTHS)
def test_row_lse_is_one_number_in_three_entry_points(V):
    x = rows_for(V)
    lse = ops.row_lse(x)
    lse2, _ = ops.row_lse_sum(x, raw=True)
    lp = ops.log_softmax_rows_(x.clone())
    torch.cuda.synchronize()
    assert torch.equal(lse, lse2), (lse.tolist(), lse2.tolist())
    # v - lse rounds once, the difference formed here once more: 2 ulp of |lse|
    back = x.cpu().numpy() - lp.cpu().numpy()
    want = lse.cpu().numpy()[:, None]
    err = np.abs(back.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    print(f"V={V}: max |x - log_softmax(x) - lse| = {err.max():.3f} ulp(lse)")
    assert np.isfinite(back).all() and err.max() <= 2.0, err.max(axis=1)


# ---------------------------------------------------------------- (b)
def pick_state(t):
    """seq, seqlp, next_tok, unfinished, n_unf of five rows in front of step t; at t = 1 row 2 has finished"""
    seq = torch.zeros(5, T_SEQ, dtype=torch.int64, device=DEV)
    seqlp = torch.zeros(5, T_SEQ, dtype=torch.float32, device=DEV)
    next_tok = torch.full((5,), -3, dtype=torch.int64, device=DEV)
    unf = torch.tensor([1, 1, 0, 1, 1] if t else [7, 7, 7, 7, 7], dtype=torch.int32, device=DEV)      # step 0 does not read it
    n_unf = torch.zeros(1, dtype=torch.int32, device=DEV)
    return seq, seqlp, next_tok, unf, n_unf


@pytest.mark.parametrize("t", [0, 1])
@pytest.mark.parametrize("raw", [False, True], ids=["logp", "raw"])
@pytest.mark.parametrize("V", WIDTHS)
def test_greedy_pick_is_one_rule_in_three_kernels(V, raw, t):
    x = rows_for(V)
    if not raw:
        x = ops.log_softmax_rows_(x)
    a, b, c = pick_state(t), pick_state(t), pick_state(t)
    ops.decode_pick(x, 0, 1.0, None, t, *a, raw=raw)
    ops.sc_pick(x, 0, 1.0, None, t, *b, raw=raw)
    first = torch.from_numpy(np.argmax(x.cpu().numpy(), axis=1).astype(np.int64)).to(DEV)           # numpy: the first of equal maxima
    given = torch.zeros(5, T_SEQ, dtype=torch.int64, device=DEV)
    given[:, t] = first
    forced.forced_pick(x, given, t, *c, raw=raw)
    torch.cuda.synchronize()
    for name, u, v in zip(("seq", "seqlp", "next_tok", "unfinished", "n_unf"), a, b):
        assert torch.equal(u, v), (name, u.tolist(), v.tolist())
    live = torch.tensor([1, 1, 0, 1, 1] if t else [1] * 5, dtype=torch.int64, device=DEV)
    assert torch.equal(a[2], first * live), (a[2].tolist(), first.tolist())
    if V > 256:
        assert int(first[3]) == 255
    for i, name in ((0, "seq"), (2, "next_tok"), (3, "unfinished")):                                # seqlp: another order of additions
        assert torch.equal(a[i], c[i]), (name, a[i].tolist(), c[i].tolist())


# ---------------------------------------------------------------- (c)
@pytest.fixture(scope="module", params=[(3, 5, 37, 0), (3, 5, 1001, 0), (2, 3, 256, 4)], ids=lambda p: "S%d-T%d-V%d-pad%d" % p)
def crit_case(request):
    """Log-probabilities, targets, a mask with one zero row, `active` with one inactive row, a reward, and the three forwards."""
    S, T, V, pad = request.param
    g = torch.Generator().manual_seed(7 * V + S)
    logp = ops.log_softmax_rows_(torch.randn(S * T, V, generator=g).to(DEV))
    target = torch.randint(0, V, (S, T), generator=g).to(DEV)
    mask = torch.ones(S, T, device=DEV)
    mask[1, 1] = 0.0
    active = torch.ones(S * T, dtype=torch.int32, device=DEV)
    active[2] = 0
    reward = (torch.randn(S, T, generator=g) + 0.5).to(DEV)
    _, slp = ops.row_lse_sum(logp, raw=False)
    lp3 = logp.view(S, T, V)
    fwd = {"plain": ops.masked_nll_fwd(lp3, target, mask),
           "smoothed": ops.smoothed_nll_fwd(lp3, target, mask, slp, 0.0),
           "reward": ops.reward_logits_fwd(lp3, target, mask, reward)}
    torch.cuda.synchronize()
    return dict(S=S, T=T, V=V, pad=pad, logp=logp, target=target, mask=mask, active=active, reward=reward, fwd=fwd)


def run_bwd(case, b16):
    """-> {rule: dlogits [S * T, V]} of the three fused backwards into buffers filled with ones beforehand"""
    S, T, V, pad = case["S"], case["T"], case["V"], case["pad"]
    dloss = torch.tensor(0.75, device=DEV)

    def buf():
        if b16:
            o = torch.ones(S * T, (V + 7) // 8 * 8 + pad, device=DEV, dtype=ops.BF16)
        else:
            o = torch.ones(S * T, V + pad, device=DEV)
        return o[:, :V]
    lp, tg, m, ac = case["logp"], case["target"], case["mask"], case["active"]
    out = {"plain": ops.nll_logsoftmax_bwd(lp, tg, m, case["fwd"]["plain"][1], dloss, buf(), ac, S, T, V),
           "smoothed": ops.smoothed_logsoftmax_bwd(lp, tg, m, case["fwd"]["smoothed"][1], dloss, 0.0, buf(), ac, S, T, V),
           "reward": ops.reward_logsoftmax_bwd(lp, tg, m, case["reward"], case["fwd"]["reward"][1], dloss, buf(), ac, S, T, V)}
    torch.cuda.synchronize()
    return out


def test_plain_and_zero_smoothing_forward_are_bit_equal(crit_case):
    (lp, sp), (ls, ss) = crit_case["fwd"]["plain"], crit_case["fwd"]["smoothed"]
    assert torch.equal(lp, ls), (lp.item(), ls.item())
    assert torch.equal(sp, ss), (sp.tolist(), ss.tolist())


@pytest.mark.parametrize("b16", [False, True], ids=["fp32", "bf16"])
def test_fused_backwards_zero_the_same_rows_and_plain_equals_zero_smoothing(crit_case, b16):
    out = run_bwd(crit_case, b16)
    dead = (crit_case["mask"].reshape(-1) == 0) | (crit_case["active"] == 0)
    assert int(dead.sum()) == 2
    for name, d in out.items():
        assert not bool(d[dead].float().ne(0).any()), name
        assert bool(d[~dead].float().ne(1).any(dim=1).all()), name                # every other row was written
    bits = torch.int16 if b16 else torch.int32
    assert torch.equal(out["plain"].contiguous().view(bits), out["smoothed"].contiguous().view(bits))
