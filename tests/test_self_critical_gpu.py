"""Self-critical sequence training on the device: the seven entry points of include/subgc_selfcritical_hip.h, the stand-alone
RewardCriterion, the rollout, the reward and the model paths (unpacked DecoderFn, packed loss-only decoder, bf16 storage) against the
fixtures the reference's own RewardCriterion, COCO scorers and model wrote and the fp64 restatements that test_self_critical_cpu.py ties to
them.  Tolerances: DESIGN 4.N (self_critical_golden.loss_bound / fused_loss_bound) for the kernels; the project's fp32 parity tolerances
(lang_loss 1e-4, gradients atol 2e-4 / rtol 2e-3) and SURVEY 8(c)'s bf16 tolerance for the model."""
import numpy as np
import pytest
import torch

import accuracy_golden as AG
import self_critical_golden as G
import bench
from subgc import accuracy, functions as F_, ops, selfcritical, synthetic
from subgc._lib import SubgcError
import subgc.models as models

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = G.U


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def host(t):
    return t.detach().float().cpu().numpy() if t.dtype == torch.bfloat16 else t.detach().cpu().numpy()


# ----------------------------------------------------------------------------------------------------------------- 1. the fixture
def test_standalone_criterion_matches_the_reference_fixture():
    meta, arr = G.load_case()
    seq = dev(arr["seq"])
    for key in meta["keys"]:
        rname, gname = key.split("_")
        inp = dev(arr["input"]).requires_grad_(True)
        gpn = dev(arr["gpn_loss"]).requires_grad_(True) if gname == "gpn" else None
        reward = dev(arr["reward_" + rname]).requires_grad_(True)
        loss = models.RewardCriterion()(inp, seq, reward, gpn)
        loss.backward()
        tol = 2 * G.loss_bound(arr["input"], arr["seq"], arr["reward_" + rname], None if gpn is None else arr["gpn_loss"])      # both sides are fp32
        got = float(loss.detach())
        print(f"{key}: loss {got:.8f} ref {float(arr['loss_' + key]):.8f} |d| {abs(got - float(arr['loss_' + key])):.2e} tol {tol:.2e}")
        assert abs(got - float(arr["loss_" + key])) <= tol, key
        np.testing.assert_allclose(host(inp.grad), arr["dinput_" + key], rtol=8 * U, atol=0, err_msg=key)
        assert reward.grad is None                                              # data, as in the reference
        if gpn is not None:
            np.testing.assert_allclose(host(gpn.grad), arr["dgpn_" + key], rtol=8 * U, atol=0, err_msg=key)


# ------------------------------------------------------------------------------------------- 2. fp64 restatement, seeded inputs
def seeded(S, T, V, seed):
    """S*T x V logits randn * 3 (fp32), targets that include 0 and V - 1, a 0/1 mask whose first column is 1, per-token rewards with
    negative and zero entries."""
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(S * T, V, generator=gen) * 3.0).float()
    tgt = torch.randint(0, V, (S, T), generator=gen)
    tgt.view(-1)[0], tgt.view(-1)[-1] = 0, V - 1
    msk = (torch.rand(S, T, generator=gen) < 0.7).float()
    msk[:, 0] = 1.0
    rwd = torch.randn(S, T, generator=gen).float()
    if S * T > 1:
        rwd.view(-1)[(S * T) // 2] = 0.0
    return x, tgt, msk, rwd


@pytest.mark.parametrize("V", [37, 256, 1001, 9488])
@pytest.mark.parametrize("T", [1, 5, 17])
@pytest.mark.parametrize("S", [1, 3, 37])
def test_fused_criterion_matches_the_fp64_restatement(S, T, V):
    """Odd V takes the one-column path, V % 4 == 0 the four-column one.  (a) fp32 log-probabilities, (b) raw logits whose lse is offset by
    +50 / -20, (c) den_override, (d) the backward in fp32 and bf16 with an inactive row: the existing NLL backward's tolerance
    (tests/test_kernels_gpu.py: atol 1e-7, rtol 1e-4; bf16 atol 2e-3 max|want|, rtol 1e-2) scaled by max|r|."""
    x, tgt, msk, rwd = seeded(S, T, V, 1000 * S + 10 * T + V)
    rows = S * T
    tn, mn, rn = tgt.numpy(), msk.numpy(), rwd.numpy()
    tgt_d, msk_d, rwd_d = tgt.to(DEV), msk.to(DEV), rwd.to(DEV)
    lp64 = G.log_softmax64(x.numpy()).reshape(S, T, V)
    lp32 = lp64.astype(np.float32)
    want, dwant = G.fused64(lp32, tn, mn, rn, dloss=0.7)
    lp_d = dev(lp32)
    loss, scratch = ops.reward_logits_fwd(lp_d, tgt_d, msk_d, rwd_d)
    tol = G.fused_loss_bound(lp32, tn, mn, rn)
    worst = [abs(float(loss) - want) / tol]
    assert abs(float(loss) - want) <= tol and float(scratch[1]) == float(msk.sum())
    for off in (50.0, -20.0):
        xo = (x + off).float()
        lpo = G.log_softmax64(xo.numpy()).reshape(S, T, V)
        lse64 = xo.double().logsumexp(1).numpy()
        xo_d = xo.to(DEV)
        lse = ops.row_lse(xo_d)
        l_raw, _ = ops.reward_logits_fwd(xo_d.view(S, T, V), tgt_d, msk_d, rwd_d, lse=lse)
        w_raw, _ = G.fused64(lpo, tn, mn, rn)
        t_raw = G.fused_loss_bound(lpo, tn, mn, rn, lse64=lse64)
        worst.append(abs(float(l_raw) - w_raw) / t_raw)
        assert abs(float(l_raw) - w_raw) <= t_raw, off
    den = torch.tensor([float(msk.sum()) + 3.0], device=DEV)
    l_den, sc_den = ops.reward_logits_fwd(lp_d, tgt_d, msk_d, rwd_d, den=den)
    w_den, _ = G.fused64(lp32, tn, mn, rn, den=float(den))
    assert abs(float(l_den) - w_den) <= G.fused_loss_bound(lp32, tn, mn, rn, den=float(den)) and float(sc_den[1]) == float(den)
    # backward
    active = torch.ones(rows, dtype=torch.int32)
    if rows > 1:
        active[rows - 1] = 0
    dwant = dwant.reshape(rows, V) * active.numpy()[:, None]
    dl = torch.tensor(0.7, device=DEV)
    rmax = float(rwd.abs().max())
    d32 = ops.reward_logsoftmax_bwd(lp_d.view(rows, V), tgt_d, msk_d, rwd_d, scratch, dl, torch.empty(rows, V, device=DEV), active.to(DEV), S, T, V)
    np.testing.assert_allclose(host(d32), dwant, atol=1e-7 * rmax, rtol=1e-4)
    d16 = ops.reward_logsoftmax_bwd(lp_d.view(rows, V), tgt_d, msk_d, rwd_d, scratch, dl, ops.empty_b16(rows, V, DEV), active.to(DEV), S, T, V)
    np.testing.assert_allclose(host(d16), dwant, atol=2e-3 * float(np.abs(dwant).max()), rtol=1e-2)
    assert torch.equal(d16.float().cpu(), d32.cpu().to(torch.bfloat16).float())     # the same arithmetic, rounded once at the store
    dead = (msk.view(-1) == 0) | (active == 0)
    assert not d32.cpu()[dead].any() and not d16.float().cpu()[dead].any()           # masked / inactive rows: exactly zero
    err = float(np.abs(host(d32) - dwant).max())
    print(f"S={S} T={T} V={V}: loss err / bound (logp, +50, -20) {worst[0]:.3f} {worst[1]:.3f} {worst[2]:.3f}  dlogits max err {err:.2e}")


@pytest.mark.parametrize("S,T", [(1, 1), (3, 5), (37, 17)])
def test_standalone_criterion_matches_the_fp64_restatement(S, T):
    gen = torch.Generator().manual_seed(7 + S)
    inp = -(torch.rand(S, T, generator=gen) * 8.0)
    seq = torch.randint(0, 4, (S, T), generator=gen) * torch.randint(1, 9000, (S, T), generator=gen)
    rwd = torch.randn(S, T, generator=gen)
    gpn = torch.rand(S, generator=gen)
    for g in (None, gpn):
        x = inp.clone().to(DEV).requires_grad_(True)
        gd = None if g is None else g.clone().to(DEV).requires_grad_(True)
        loss = models.RewardCriterion()(x, seq.to(DEV), rwd.to(DEV), gd)
        (loss * 0.7).backward()
        want, dinp, dgpn = G.criterion64(inp.numpy(), seq.numpy(), rwd.numpy(), None if g is None else g.numpy(), dloss=0.7)
        tol = G.loss_bound(inp.numpy(), seq.numpy(), rwd.numpy(), None if g is None else g.numpy())
        got = float(loss.detach())
        print(f"S={S} T={T} gpn={g is not None}: |d| {abs(got - want):.2e} tol {tol:.2e}")
        assert abs(got - want) <= tol
        np.testing.assert_allclose(host(x.grad), dinp, rtol=8 * U, atol=0)
        if g is not None:
            np.testing.assert_allclose(host(gd.grad), dgpn, rtol=8 * U, atol=0)


@pytest.mark.parametrize("S,T,V", [(3, 5, 37), (37, 17, 256), (3, 17, 9488), (37, 5, 1001)])
def test_reward_one_is_the_masked_nll_and_reward_zero_is_zero(S, T, V):
    x, tgt, _, _ = seeded(S, T, V, 5 + V)
    seq = tgt.clone()
    seq[0, T // 2:] = 0
    mask = torch.from_numpy(G.mask_of(seq.numpy())).float().to(DEV)               # the shifted mask of RewardCriterion
    lp = torch.log_softmax(x, 1).to(DEV)
    tgt_d, rows = seq.to(DEV), S * T
    dl = torch.tensor(0.7, device=DEV)
    one, zero = torch.ones(S, T, device=DEV), torch.zeros(S, T, device=DEV)
    l_nll, sc_nll = ops.masked_nll_fwd(lp.view(S, T, V), tgt_d, mask)
    d_nll = ops.nll_logsoftmax_bwd(lp, tgt_d, mask, sc_nll, dl, torch.empty(rows, V, device=DEV), None, S, T, V)
    l_one, sc_one = ops.reward_logits_fwd(lp.view(S, T, V), tgt_d, mask, one)
    d_one = ops.reward_logsoftmax_bwd(lp, tgt_d, mask, one, sc_one, dl, torch.empty(rows, V, device=DEV), None, S, T, V)
    rel = abs(float(l_one) - float(l_nll)) / abs(float(l_nll))
    print(f"S={S} T={T} V={V}: reward 1 vs NLL, loss rel {rel / U:.2f} u, dlogits max rel "
          f"{float(((d_one - d_nll).abs() / d_nll.abs().clamp_min(1e-30)).max()) / U:.2f} u")
    assert rel <= 8 * U
    np.testing.assert_allclose(host(d_one), host(d_nll), rtol=8 * U, atol=0)
    l_zero, sc_zero = ops.reward_logits_fwd(lp.view(S, T, V), tgt_d, mask, zero)
    d_zero = ops.reward_logsoftmax_bwd(lp, tgt_d, mask, zero, sc_zero, dl, torch.empty(rows, V, device=DEV), None, S, T, V)
    assert float(l_zero) == 0.0 and not d_zero.any()
    # the stand-alone class on the gathered log-probabilities is the same loss
    l_alone = models.RewardCriterion()(lp.view(S, T, V).gather(2, tgt_d.unsqueeze(2)).squeeze(2), tgt_d, one)
    assert abs(float(l_alone) - float(l_one)) <= 8 * U * abs(float(l_one))


def test_criterion_launches_are_bit_reproducible_with_and_without_deterministic_mode():
    S, T, V = 5, 7, 1001
    x, tgt, msk, rwd = seeded(S, T, V, 31)
    xd, tgt, msk, rwd = x.to(DEV), tgt.to(DEV), msk.to(DEV), rwd.to(DEV)
    dl = torch.tensor(0.9, device=DEV)

    def run():
        lse = ops.row_lse(xd)
        loss, sc = ops.reward_logits_fwd(xd.view(S, T, V), tgt, msk, rwd, lse=lse)
        d = ops.reward_logsoftmax_bwd(xd, tgt, msk, rwd, sc, dl, torch.empty(S * T, V, device=DEV), None, S, T, V, lse=lse)
        inp = xd.view(S, T, V)[:, :, 0].contiguous()
        l2, sc2 = ops.reward_nll_fwd(inp, tgt, rwd, rwd[:, 0].contiguous())
        return (loss, sc, d, l2, sc2) + ops.reward_nll_bwd(tgt, rwd, rwd[:, 0].contiguous(), sc2, dl)

    a, b = run(), run()
    with ops.deterministic():
        c = run()
    for p, q, r in zip(a, b, c):
        assert torch.equal(p, q) and torch.equal(p, r)


# ------------------------------------------------------------------------------------------------------------------ 3. the pick
def pick_state(n, T):
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device=DEV, dtype=dt)
    return z(n, T, dt=torch.long), z(n, T), z(n, dt=torch.long), z(n, dt=torch.int32), z(T, dt=torch.int32)


@pytest.mark.parametrize("temp", [1.0, 0.7])
@pytest.mark.parametrize("V", [37, 1001, 9488, 16384])
@pytest.mark.parametrize("n", [1, 2, 5, 300])
def test_sc_pick_draws_by_inverse_cdf_and_keeps_decode_picks_greedy_rows(n, V, temp):
    """Every n_sample in 0 .. n.  Sampling rows: u sits at the midpoint of the fp64 CDF interval of a chosen token of probability >= 1e-4;
    the half-width of >= 5e-5 is far above the fp32 CDF's error of about (ceil(V / 256) + 14) u, so every draw must be that token.
    Greedy rows: subgc_decode_pick(k = 0) on the same logits, bit for bit, on raw logits and on log-probabilities."""
    T = 3
    gen = torch.Generator().manual_seed(17 * n + V)
    x = (torch.randn(n, V, generator=gen) * 2.0).float()
    x[n // 2, 0] = 30.0                                                          # this row ends at once, drawn or greedy
    p = torch.softmax(x.double() / temp, 1)
    cdf = p.cumsum(1)
    chosen = torch.zeros(n, dtype=torch.long)
    u = torch.zeros(n)
    for r in range(n):
        ok = (p[r] >= 1e-4).nonzero().view(-1)
        c = int(ok[int(torch.randint(0, len(ok), (1,), generator=gen))])
        chosen[r] = c
        u[r] = float((cdf[r, c] - 0.5 * p[r, c]))
    assert int(chosen[n // 2]) == 0
    lp_want = torch.log_softmax(x.double() / temp, 1).gather(1, chosen.view(-1, 1)).view(-1)
    xd, ud = x.to(DEV), u.to(DEV)
    for raw in (True, False):
        src = xd if raw else torch.log_softmax(xd, 1)
        gs, gl, gi, gu, gc = pick_state(n, T)
        ops.decode_pick(src, 0, 1.0, None, 0, gs, gl, gi, gu, gc[0:1], None, raw=raw)
        rows = torch.arange(n, device=DEV)
        for n_sample in range(n + 1):
            s, l, it, unf, cnt = pick_state(n, T)
            ops.sc_pick(src, n_sample, temp, ud, 0, s, l, it, unf, cnt[0:1], None, raw=raw)
            samp = rows < n_sample
            want_tok = torch.where(samp, chosen.to(DEV), gs[:, 0])
            assert torch.equal(s[:, 0], want_tok), (n_sample, raw)
            assert torch.equal(l[:, 0][~samp], gl[:, 0][~samp])                  # greedy lp: the same bits
            assert torch.equal(it, want_tok) and torch.equal(unf, (want_tok > 0).int())
            assert (int(cnt[0]) != 0) == bool((want_tok > 0).any())
            if n_sample in (n, n // 2 + 1):
                np.testing.assert_allclose(host(l[:n_sample, 0]), lp_want[:n_sample].numpy(), atol=1e-5, rtol=0)
                s2, l2, it2, unf2, cnt2 = pick_state(n, T)                       # two launches: equal bits
                ops.sc_pick(src, n_sample, temp, ud, 0, s2, l2, it2, unf2, cnt2[0:1], None, raw=raw)
                assert torch.equal(s, s2) and torch.equal(l, l2)
                # step 1: a finished row stays at 0
                ops.sc_pick(src.roll(1, 1).contiguous(), n_sample, temp, ud, 1, s, l, it, unf, cnt[1:2], cnt[0:1], raw=raw)
                assert int(s[n // 2, 1]) == 0 and int(unf[n // 2]) == 0 and int(it[n // 2]) == 0
                before = (s.clone(), l.clone(), it.clone(), unf.clone())
                zero = torch.zeros(1, dtype=torch.int32, device=DEV)
                ops.sc_pick(src, n_sample, temp, ud, 2, s, l, it, unf, cnt[2:3], zero, raw=raw)      # prev_count == 0: nothing is written
                assert all(torch.equal(a, b) for a, b in zip(before, (s, l, it, unf))) and int(cnt[2]) == 0


@pytest.mark.parametrize("V", [37, 1001, 16384])
def test_sc_pick_edges_of_the_unit_interval_and_a_one_hot_row(V):
    gen = torch.Generator().manual_seed(V)
    x = (torch.randn(4, V, generator=gen) * 2.0).float()
    x[2] = -float("inf"); x[2, V // 3] = 0.0                                     # one-hot rows
    x[3] = -float("inf"); x[3, V - 1] = 1.5
    xd = x.to(DEV)
    for uval in (0.0, 1.0 - 2.0 ** -24, 0.37):
        s, l, it, unf, cnt = pick_state(4, 2)
        ops.sc_pick(xd, 4, 1.0, torch.full((4,), uval, device=DEV), 0, s, l, it, unf, cnt[0:1], None, raw=True)
        got = s[:, 0].cpu().tolist()
        assert got[2:] == [V // 3, V - 1] and float(l[2, 0]) == 0.0 and float(l[3, 0]) == 0.0
        eps = (-(-V // 256) + 14) * U                                           # the fp32 CDF's error: the pick's interval holds u up to that
        for r in range(2):
            c = G.cdf64(x[r].numpy())
            uu = float(np.float32(uval))
            assert c[got[r]] > uu - eps and (got[r] == 0 or c[got[r] - 1] <= uu + eps), (uval, r, got[r])
        if uval == 0.0:
            assert got[:2] == [0, 0]                                             # randn * 2: the first column's mass does not underflow
        if uval == 0.37:
            assert got[:2] == [G.inv_cdf_pick(x[r].numpy(), np.float32(uval)) for r in range(2)] or min(
                G.boundary_distance(x[r].numpy(), np.float32(uval)) for r in range(2)) < eps
    s, l, it, unf, cnt = pick_state(4, 2)                                        # u == NULL draws with 0
    ops.sc_pick(xd, 4, 1.0, None, 0, s, l, it, unf, cnt[0:1], None, raw=True)
    assert s[:, 0].cpu().tolist()[2:] == [V // 3, V - 1]


# ------------------------------------------------------------------------------------------------------- 4. prepare and reward
def test_sc_prepare_writes_labels_mask_and_scored_rows():
    meta, arr = G.load_case()
    cand = arr["cand"]
    eos = meta["V"] + 1
    labels, mask, rows = ops.sc_prepare(dev(cand), eos + 1, eos)
    lab, m = G.replay_labels(cand)
    assert np.array_equal(host(labels), lab) and np.array_equal(host(mask), m) and np.array_equal(host(rows), G.eos_rows(cand, eos))
    _, _, plain = ops.sc_prepare(dev(cand), eos + 1, 0, want_replay=False)
    assert np.array_equal(host(plain)[:, :-1], cand) and not host(plain)[:, -1].any()
    dirty = cand.copy(); dirty[5, 3] = 0; dirty[5, 4] = 9                         # words behind the first 0 are not scored
    _, _, rows = ops.sc_prepare(dev(dirty), eos + 1, eos, want_replay=False)
    assert np.array_equal(host(rows), G.eos_rows(dirty, eos)) and not host(rows)[5, 4:].any()


@pytest.mark.parametrize("wc,wb", [(1.0, 0.0), (0.0, 1.0), (1.0, 0.5)])
def test_reward_matches_the_reference_scorers(wc, wb):
    meta, arr = G.load_case()
    refs = selfcritical.RewardReferences(G.per_image(arr["ref_rows"], arr["ref_cap_off"]))
    rw = selfcritical.SelfCriticalReward(refs, wc, wb)
    S, T = 20, meta["L"]
    reward, mean_reward, scores = rw.enqueue(dev(arr["cand"]), dev(arr["cand_img"], torch.int32))
    torch.cuda.synchronize()
    cider, bleu4 = arr["cider"], arr["bleu"][:, 3]
    got = host(scores)
    if wb == 0.0:
        assert AG.rel(got, cider) <= AG.CIDER_TOL
    if wc == 0.0:
        assert AG.rel(got, bleu4) <= AG.BLEU_TOL
    a_c, a_b = AG.CIDER_TOL * np.abs(cider).max(), AG.BLEU_TOL * np.abs(bleu4).max()
    want_s = wc * cider + wb * bleu4
    assert np.abs(got - want_s).max() <= wc * a_c + wb * a_b + 1e-16
    want_r = want_s[:S] - want_s[S:]
    r = host(reward)
    assert r.shape == (S, T + 1) and (r == r[:, :1]).all()                       # constant along t
    assert (np.abs(r[:, 0] - want_r) <= (wc + wb) * 2 * max(a_c, a_b) + U * np.abs(want_r)).all()
    assert abs(float(mean_reward) - r[:, 0].astype(np.float64).mean()) <= U * np.abs(r[:, 0]).max()
    print(f"w=({wc}, {wb}): score err {np.abs(got - want_s).max():.2e}, reward err {np.abs(r[:, 0] - want_r).max():.2e}, mean {float(mean_reward):.6f}")


def test_reward_without_the_end_token_is_the_accuracy_scorers_own():
    meta, arr = G.load_case()
    per = G.per_image(arr["ref_rows"], arr["ref_cap_off"])
    refs = selfcritical.RewardReferences(per, eos=False)
    cand, img = dev(arr["cand"]), arr["cand_img"]
    _, _, s_c = selfcritical.SelfCriticalReward(refs, 1.0, 0.0).enqueue(cand, dev(img, torch.int32))
    _, _, s_b = selfcritical.SelfCriticalReward(refs, 0.0, 1.0).enqueue(cand, dev(img, torch.int32))
    img2 = [int(j) for j in img] * 2
    out = accuracy.AccuracyScorer(refs, 1).score(cand, list(range(41)), img2)
    vals = np.array([e["values"][0] for e in out])
    assert np.array_equal(host(s_c), vals[:, 4]) and np.array_equal(host(s_b), vals[:, 3])


# ------------------------------------------------------------------------------------------------------------- 5. debug bounds
def test_debug_bounds_reports_a_token_id_equal_to_V_and_n_sample_beyond_n():
    S, T, V = 2, 3, 20
    x, tgt, msk, rwd = seeded(S, T, V, 5)
    lp = torch.log_softmax(x, 1).to(DEV)
    tgt = tgt.clone(); tgt[1, 1] = V
    tgt, msk, rwd = tgt.to(DEV), msk.to(DEV), rwd.to(DEV)
    one = torch.ones((), device=DEV)
    with ops.debug_bounds():
        with pytest.raises(SubgcError, match=r"reward_logits_fwd: target \(word ids\)"):
            ops.reward_logits_fwd(lp.view(S, T, V), tgt, msk, rwd)
        with pytest.raises(SubgcError, match=r"reward_logsoftmax_bwd: target \(word ids\)"):
            ops.reward_logsoftmax_bwd(lp, tgt, msk, rwd, torch.ones(2, device=DEV), one, torch.empty(S * T, V, device=DEV), None, S, T, V)
        seq2 = torch.zeros(4, 5, dtype=torch.long, device=DEV); seq2[3, 2] = V
        with pytest.raises(SubgcError, match=r"sc_prepare: seq2 \(word ids\)"):
            ops.sc_prepare(seq2, V, V + 1)
        s, l, it, unf, cnt = pick_state(S * T, 2)
        with pytest.raises(SubgcError, match=r"sc_pick: n_sample = 7 of n = 6 rows"):
            ops.sc_pick(lp, S * T + 1, 1.0, None, 0, s, l, it, unf, cnt[0:1], None)
    loss, _ = ops.reward_logits_fwd(lp.view(S, T, V), tgt, msk, rwd)             # mode off: clamped like the NLL kernels clamp it
    assert torch.isfinite(loss)
    with pytest.raises(SubgcError, match=r"sc_pick: n_sample = 7 of n = 6 rows"):   # the row count is refused in either mode
        ops.sc_pick(lp, S * T + 1, 1.0, None, 0, s, l, it, unf, cnt[0:1], None)


# ------------------------------------------------------------------------------------------------------------------- model level
def build(g, weights, **over):
    m = models.setup(g.opt(caption_model="topdown", gpn_drop_prob=0.0, **over))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    return m.to(DEV).train()


def fixture_reward(z, vocab=50):
    refs = selfcritical.RewardReferences(G.per_image(z["sc.ref_rows"], z["sc.ref_cap_off"]), vocab_size=vocab)
    wc, wb = z["sc.weights"]
    return selfcritical.SelfCriticalReward(refs, float(wc), float(wb))


def run_sc(m, batch, rw, gt_indices, seq2=None, packed=None, sc_flag=True):
    if packed is not None:
        m.packed_decoder = packed
    m.injected_sc = None if seq2 is None else dev(seq2)
    lw = models.LossWrapper(m, None, sc_reward=rw)
    b = {k: v.to(DEV) for k, v in batch.items()}
    args = list(bench.lw_args(b))
    args[6] = torch.as_tensor(np.asarray(gt_indices))
    m.flatten_grads()
    out = lw(*args, sc_flag=True) if sc_flag else lw(*args)
    if packed is not None:                                                      # the path asked for is the path that ran
        assert ("Packed" in type(out["lang_loss"].grad_fn).__name__) == bool(packed), type(out["lang_loss"].grad_fn).__name__
    models.total_loss(out).backward()
    torch.cuda.synchronize()
    return out


def close(a, b, name, atol, rtol):
    a = a.detach().float().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    np.testing.assert_allclose(a, np.asarray(b), atol=atol, rtol=rtol, err_msg=name)


@pytest.mark.parametrize("packed", [True, False])
def test_model_matches_the_reference_trained_with_the_reward_criterion(golden, packed):
    """The reference model teacher-forced on the fixture's sampled tokens with RewardCriterion and the fixture's rewards
    (self_critical_train.npz): lang_loss within 1e-4, every live gradient within atol 2e-4 / rtol 2e-3, through both decoder Functions;
    the reward itself is scored on the device from the injected rollout."""
    g, z = golden("subgc_train"), G.load_train()
    m = build(g, g.group("weights"))
    out = run_sc(m, g.tensors("inputs"), fixture_reward(z), z["sc.gt_indices"], z["sc.seq2"], packed)
    print(f"packed={packed}: lang_loss {float(out['lang_loss']):.7f} ref {float(z['lang_loss']):.7f} reward {float(out['reward']):.7f} ref {float(z['sc.mean_reward']):.7f}")
    assert set(out) == {"gpn_loss", "lang_loss", "reward"} and out["lang_loss"] is m.fused_lang_loss
    assert abs(float(out["reward"]) - float(z["sc.mean_reward"])) <= 4 * U * np.abs(z["sc.reward"]).max()
    assert m.sc_stats["reward"] is out["reward"] and np.array_equal(host(m.sc_stats["seq"]), z["sc.seq2"])
    close(out["lang_loss"], z["lang_loss"], "lang_loss", atol=1e-4, rtol=1e-4)
    close(out["gpn_loss"], z["gpn_loss"], "gpn_loss", atol=1e-4, rtol=1e-4)
    dead = set(g.meta["dead_params"])
    for k, p in m.named_parameters():
        if k in dead:
            assert float(p.grad.abs().max()) == 0.0, k
        else:
            close(p.grad, z[k], "grad " + k, atol=2e-4, rtol=2e-3)


def seeded_rollout(b5, T, V, seed):
    rng = np.random.default_rng(seed)
    seq2 = rng.integers(1, V + 1, (2 * b5, T))
    for r in range(2 * b5):
        n = int(rng.integers(0, T + 1))
        seq2[r, n:] = 0
    seq2[1] = rng.integers(1, V + 1, T)
    refs = [np.stack([seq2[int(rng.integers(0, 2 * b5))] for _ in range(2)]) for _ in range(3)]
    return seq2.astype(np.int64), refs


@pytest.mark.parametrize("name", ["subgc_train", "fullgc_train"])
def test_packed_equals_unpacked_equals_the_standalone_criterion(golden, name):
    """The sGPN and the Full-GC golden models on a seeded rollout: the two decoder Functions agree as tests/test_packed_gpu.py requires of
    them, and both losses equal the stand-alone RewardCriterion on the unpacked path's own outputs, gathered, within the derived bounds
    (the fused and the stand-alone form each against fp64)."""
    with ops.deterministic():                                                   # the three forwards then share their bits
        _packed_unpacked_standalone(golden(name), name)


def _packed_unpacked_standalone(g, name):
    m = build(g, g.group("weights"))
    batch = g.tensors("inputs")
    b5, T, V = batch["labels"].size(0), batch["labels"].size(1) - 2, m.vocab_size
    seq2, refs = seeded_rollout(b5, T, V, 3)
    rw = selfcritical.SelfCriticalReward(selfcritical.RewardReferences(refs, vocab_size=V), 1.0, 0.5)
    idx = [1, 2, 0][:g.meta["B"]] if g.meta["B"] <= 3 else list(np.arange(g.meta["B"]) % 3)
    res = {}
    for packed in (False, True):
        out = run_sc(m, batch, rw, idx, seq2, packed)
        res[packed] = (float(out["lang_loss"]), m.flat_grads.clone())
    (l0, g0), (l1, g1) = res[False], res[True]
    assert abs(l0 - l1) < 2e-5 * max(1.0, abs(l0))
    scale = float(g0.abs().max())
    np.testing.assert_allclose(g1.cpu().numpy(), g0.cpu().numpy(), atol=2e-5 * scale + 1e-7, rtol=2e-4)
    reward, _, _ = rw.enqueue(dev(seq2), dev(np.asarray(idx), torch.int32))
    lab, msk = G.replay_labels(seq2)
    fed = {k: v.to(DEV) for k, v in batch.items()}
    fed["labels"] = dev(lab)
    with torch.no_grad():
        outputs, _, _ = m(*synthetic.forward_args(fed))
    seq = dev(seq2[:b5])
    gathered = outputs[:, :T].gather(2, seq.unsqueeze(2)).squeeze(2)
    alone = float(models.RewardCriterion()(gathered, seq, reward[:, :T].contiguous()))
    lp = host(outputs)
    tol = G.fused_loss_bound(lp, lab[:, 1:], msk, host(reward)) + G.loss_bound(host(gathered), seq2[:b5], host(reward)[:, :T])
    print(f"{name}: unpacked {l0:.8f} packed {l1:.8f} stand-alone {alone:.8f} tol {tol:.2e}")
    assert abs(l0 - alone) <= tol and abs(l0) > 1e-3


@pytest.mark.parametrize("packed", [True, False])
def test_bf16_storage_path_follows_the_fp32_path(golden, packed):
    """compute_dtype = bf16 against the fp32 HIP path on the same weights, batch and injected rollout, at SURVEY 8(c)'s bf16 tolerance as
    tests/test_bf16_storage_gpu.py applies it to this golden case: loss atol 5e-2; gradients by direction and norm."""
    g, z = golden("subgc_train"), G.load_train()
    cos = lambda a, b: float((a.double().flatten() @ b.double().flatten()) / (a.double().norm() * b.double().norm() + 1e-30))
    ref_m = build(g, g.group("weights"))
    ref = run_sc(ref_m, g.tensors("inputs"), fixture_reward(z), z["sc.gt_indices"], z["sc.seq2"], packed)
    m = build(g, g.group("weights"), compute_dtype="bf16")
    assert m.bf16_storage
    out = run_sc(m, g.tensors("inputs"), fixture_reward(z), z["sc.gt_indices"], z["sc.seq2"], packed)
    print(f"packed={packed}: bf16 {float(out['lang_loss']):.6f} fp32 {float(ref['lang_loss']):.6f}")
    assert abs(float(out["lang_loss"]) - float(ref["lang_loss"])) <= 5e-2
    assert float(out["lang_loss"]) != float(ref["lang_loss"])                   # bf16 arithmetic really ran
    assert float(out["reward"]) == float(ref["reward"])                         # the reward is scored in fp64 from the same tokens
    dead, worst = set(g.meta["dead_params"]), 1.0
    for (k, p), (_, r) in zip(m.named_parameters(), ref_m.named_parameters()):
        if k in dead:
            assert float(p.grad.abs().max()) == 0.0, k
        elif float(r.grad.abs().max()) > 1e-6:
            c = cos(p.grad, r.grad)
            worst = min(worst, c)
            if k in ("logit.weight", "core.lang_lstm.weight_ih", "core.att_lstm.weight_hh", "embed.0.weight"):
                assert c > 0.995, (k, c)
                assert abs(float(p.grad.norm()) / float(r.grad.norm()) - 1.0) < 0.1, k
    assert worst > 0.95, worst


def test_two_self_critical_steps_from_the_same_seed_give_equal_bits(golden):
    """Deterministic mode, free-running rollout: the same torch seed and call count give the same tokens, loss and gradients; another
    `_sample_calls` count gives another rollout."""
    g, z = golden("subgc_train"), G.load_train()
    m = build(g, g.group("weights"))
    rw = fixture_reward(z)
    res = []
    with ops.deterministic():
        for calls in (0, 0, 1):
            torch.manual_seed(11)
            m.__dict__["_sample_calls"] = calls
            m._dropout_calls = 0
            out = run_sc(m, g.tensors("inputs"), rw, z["sc.gt_indices"])
            res.append((m.sc_stats["seq"].clone(), out["lang_loss"].clone(), out["reward"].clone(), m.flat_grads.clone()))
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
    assert not torch.equal(res[0][0], res[2][0])
    assert torch.equal(res[0][0][15:], res[2][0][15:])                           # the greedy half does not depend on the draws


@pytest.mark.parametrize("packed", [True, False])
def test_sc_flag_false_is_bit_identical_to_sc_flag_omitted(golden, packed):
    g, z = golden("subgc_train"), G.load_train()
    m = build(g, g.group("weights"))
    res = []
    with ops.deterministic():
        for rw, flag in ((None, None), (None, False), (fixture_reward(z), False)):
            m.packed_decoder = packed
            lw = models.LossWrapper(m, None, sc_reward=rw)
            b = {k: v.to(DEV) for k, v in g.tensors("inputs").items()}
            m.flatten_grads()
            out = lw(*bench.lw_args(b)) if flag is None else lw(*bench.lw_args(b), sc_flag=flag)
            assert set(out) == {"gpn_loss", "lang_loss"}
            models.total_loss(out).backward()
            torch.cuda.synchronize()
            res.append((out["lang_loss"].clone(), m.flat_grads.clone()))
    for loss, grads in res[1:]:
        assert torch.equal(loss, res[0][0]) and torch.equal(grads, res[0][1])
    close(res[0][0], g.group("out")["lang_loss"], "lang_loss", atol=1e-4, rtol=1e-4)


# ------------------------------------------------------------------------------------------------------------------- the rollout
def test_rollout_greedy_half_is_the_batched_greedy_decode_and_sampled_half_is_the_inverse_cdf(golden, monkeypatch):
    """On the subgc_train golden model.  The rollout's arguments are taken from a real self-critical step.  (a) The greedy half equals the
    existing batched greedy decode (functions.DecodeState + subgc_decode_pick, as models/sampling.py runs it) of the same sub-graphs in
    the same batch, token for token.  (b) The sampled half: the rollout's own tokens are forced through the decode step to get every
    step's row, and each live draw must be the fp64 inverse-CDF pick for its u; a draw whose u lies within 1e-5 of a CDF boundary may
    be skipped, at most 1 % of the live draws (expected share <= 2e-5 * 50, test_self_critical_cpu.py)."""
    g, z = golden("subgc_train"), G.load_train()
    m = build(g, g.group("weights"))
    T, b5 = 16, 15                                                              # the loader's caption width, not the decode length
    gen = torch.Generator().manual_seed(99)
    u = torch.rand(T, b5, generator=gen).to(DEV)
    seen = {}
    real = selfcritical.rollout

    def spy(model, fc, Xb, lens, sel_idx, img_s, N, uniforms=None, T=None):
        seen.update(fc=fc.detach().clone(), Xb=Xb.detach().clone(), lens=lens.clone(), sel_idx=sel_idx.clone(), img_s=img_s.clone(), N=N)
        seen["seq2"] = real(model, fc, Xb, lens, sel_idx, img_s, N, uniforms=u, T=T)
        return seen["seq2"]

    monkeypatch.setattr(selfcritical, "rollout", spy)
    out = run_sc(m, g.tensors("inputs"), fixture_reward(z), z["sc.gt_indices"])
    seq2 = seen["seq2"]
    assert seq2.shape == (2 * b5, T) and seq2.dtype == torch.int64 and torch.isfinite(out["lang_loss"]) and int(seq2.max()) <= m.vocab_size
    two = lambda t: torch.cat([t, t]).contiguous()
    P = [p.detach() for p in m._decoder_params()]
    with torch.no_grad():
        # (a) all 2 * b5 rows greedy
        pr = F_.Prepared(two(seen["fc"]), seen["Xb"], two(seen["lens"]), two(seen["sel_idx"]), two(seen["img_s"]), seen["N"], P, None, None, 1.0)
        st = F_.DecodeState(pr, P, seen["N"], False, xt_table=m.xt_gates_table(), fuse_lstm=True, snapshots=m.decode_snapshots(), W16=m.decode_w16())
        s, l, it, unf, cnt = pick_state(2 * b5, T)
        for t in range(T):
            logits = st.step(it, None, normalize=False)
            ops.decode_pick(logits, 0, 1.0, None, t, s, l, it, unf, cnt[t:t + 1], cnt[t - 1:t] if t > 0 else None, raw=True)
        assert torch.equal(s[b5:], seq2[b5:]) and torch.equal(s[:b5], s[b5:]) and bool(s.any())
        # (b) the sampled tokens forced through the same state
        st.reset()
        it = torch.zeros(2 * b5, dtype=torch.long, device=DEV)
        rows = []
        for t in range(T):
            rows.append(st.step(it, None, normalize=False)[:b5].double().cpu().numpy())
            it = two(seq2[:b5, t]).contiguous()
    tok, uu = seq2[:b5].cpu().numpy(), u.cpu().numpy()
    live = skipped = 0
    for sidx in range(b5):
        for t in range(T):
            if t > 0 and tok[sidx, t - 1] == 0:
                break
            live += 1
            if G.boundary_distance(rows[t][sidx], uu[t, sidx]) < 1e-5:
                skipped += 1
                continue
            assert tok[sidx, t] == G.inv_cdf_pick(rows[t][sidx], uu[t, sidx]), (sidx, t)
    print(f"rollout: {live} live draws, {skipped} skipped near a boundary; greedy half {int((seq2[b5:] > 0).sum())} words")
    assert live >= b5 and skipped <= 0.01 * live
    assert not torch.equal(seq2[:b5], seq2[b5:])                                # the sampled half really sampled


def test_free_running_step_at_bench_width_under_debug_bounds():
    """A self-critical step of the bench's Sub_GC_Kar model (8 images) with the model's own Philox stream, every index tensor checked:
    finite loss and gradients, rollout ids below V, the decoder ran packed."""
    import argparse
    torch.manual_seed(3)
    m = models.setup(argparse.Namespace(**bench.KAR)).to(DEV).train()
    B = 8
    batch = synthetic.make_train_batch(B, seed=5)
    rng = np.random.default_rng(1)
    W = batch["labels"].size(1) - 2
    refs = [rng.integers(0, m.vocab_size + 1, (5, W)) * (np.arange(W) < rng.integers(4, W + 1, (5, 1))) for _ in range(B)]
    rw = selfcritical.SelfCriticalReward(selfcritical.RewardReferences(refs, vocab_size=m.vocab_size), 1.0, 0.0)
    with ops.debug_bounds():
        out = run_sc(m, batch, rw, list(range(B)))
    seq2 = m.sc_stats["seq"]
    assert "Packed" in type(out["lang_loss"].grad_fn).__name__
    assert torch.isfinite(out["lang_loss"]) and torch.isfinite(out["reward"]) and bool(torch.isfinite(m.flat_grads).all())
    assert seq2.shape == (2 * batch["labels"].size(0), W) and int(seq2.min()) >= 0 and int(seq2.max()) < m.vocab_size + 1
    assert float(m.flat_grads.abs().max()) > 0
