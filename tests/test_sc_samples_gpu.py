"""The one-pass self-critical step on the device (`LossWrapper(..., sc_samples=n)`, n >= 2): n samples per caption row drawn inside the
decoder Function's own forward, the leave-one-out reward, RewardCriterion on the logits the draws were made from.  Golden tiny models
(b5 = 15, T = 16, V = 50), fixtures of tests/golden/make_golden_sc_samples.py.  Tolerances: the project's model-level ones (lang_loss 1e-4,
gradients atol 2e-4 / rtol 2e-3) against the reference; the two-routes tolerance of test_packed_equals_unpacked_equals_the_standalone_
criterion (loss 2e-5, gradients atol 2e-5 max|g| + 1e-7 / rtol 2e-4) against the two-pass step; bits where the arithmetic is the same."""
import numpy as np
import pytest
import torch

import accuracy_golden as AG
import sc_samples_golden as SG
import self_critical_golden as G
import test_self_critical_gpu as SCG
import bench
from subgc import ops, selfcritical
import subgc.models as models

pytestmark = pytest.mark.gpu
DEV = SCG.DEV
U = G.U
dev, host = SCG.dev, SCG.host
IDX = [2, 0, 1]


def step(m, batch, rw, gt_indices, n, tokens=None, u=None, sc_flag=True, **lw_kw):
    """One training step through LossWrapper; -> (out, flat gradient clone)."""
    m.injected_sc = None if tokens is None else (tokens if torch.is_tensor(tokens) else dev(tokens))
    m.injected_sc_u = u
    if n is not None:
        lw_kw["sc_samples"] = n
    lw = models.LossWrapper(m, lw_kw.pop("opt", None), sc_reward=rw, **lw_kw)
    b = {k: v.to(DEV) for k, v in batch.items()}
    args = list(bench.lw_args(b))
    args[6] = torch.as_tensor(np.asarray(gt_indices))
    m.flatten_grads()
    out = lw(*args, sc_flag=True) if sc_flag else lw(*args)
    models.total_loss(out).backward()
    torch.cuda.synchronize()
    m.injected_sc = m.injected_sc_u = None
    return out, m.flat_grads.clone()


def case_reward(z, pre, vocab=50):
    refs = selfcritical.RewardReferences(G.per_image(z[pre + "sc.ref_rows"], z[pre + "sc.ref_cap_off"]), vocab_size=vocab)
    wc, wb = z[pre + "sc.weights"]
    return selfcritical.SelfCriticalReward(refs, float(wc), float(wb))


def seeded_reward(b5, T, V, seed=3):
    _, refs = SCG.seeded_rollout(b5, T, V, seed)
    return selfcritical.SelfCriticalReward(selfcritical.RewardReferences(refs, vocab_size=V), 1.0, 0.5)


def live_steps(tok):
    """[(row, t)] of the steps at which a row still draws: t = 0, and every t whose previous token is no end token."""
    return [(r, t) for r in range(tok.shape[0]) for t in range(tok.shape[1]) if t == 0 or tok[r, :t].all()]


# ------------------------------------------------------------------------------------------------------ 1. the reference's fixture
@pytest.mark.parametrize("n", SG.NS_TRAIN)
@pytest.mark.parametrize("name", SG.MODELS)
def test_injected_tokens_give_the_reference_models_loss_and_gradients(golden, name, n):
    g, z, pre = golden(name), SG.load("sc_samples_train.npz"), f"{name}.n{n}."
    m = SCG.build(g, g.group("weights"))
    tok = z[pre + "sc.tok"]
    out, _ = step(m, g.tensors("inputs"), case_reward(z, pre), z[pre + "sc.gt_indices"], n, tokens=tok)
    st = m.sc_stats
    S, T = tok.shape
    print(f"{name} n={n}: lang_loss {float(out['lang_loss']):.7f} ref {float(z[pre + 'lang_loss']):.7f} reward {float(out['reward']):.3e}")
    assert set(out) == {"gpn_loss", "lang_loss", "reward"} and out["lang_loss"] is m.fused_lang_loss and out["reward"] is st["reward"]
    assert np.array_equal(host(st["seq"]), tok) and st["scores"].dtype == st["baseline"].dtype == torch.float64
    assert st["scores"].shape == st["baseline"].shape == (S,) and st["rewards"].shape == (S, T + 1)
    a_c = AG.CIDER_TOL * np.abs(z[pre + "sc.scores"]).max() + AG.BLEU_TOL
    assert np.abs(host(st["scores"]) - z[pre + "sc.scores"]).max() <= a_c
    assert np.abs(host(st["rewards"])[:, 0] - z[pre + "sc.reward"]).max() <= 4 * a_c + U * np.abs(z[pre + "sc.reward"]).max()
    SCG.close(out["lang_loss"], z[pre + "lang_loss"], "lang_loss", atol=1e-4, rtol=1e-4)
    if pre + "gpn_loss" in z:
        SCG.close(out["gpn_loss"], z[pre + "gpn_loss"], "gpn_loss", atol=1e-4, rtol=1e-4)
    dead, seen = set(g.meta["dead_params"]), 0
    for k, p in m.named_parameters():
        if k in dead:
            assert float(p.grad.abs().max()) == 0.0, k
            continue
        idx = SG.sample_index(k, p.numel())
        if idx is None:
            SCG.close(p.grad, z[pre + "grad." + k], "grad " + k, atol=2e-4, rtol=2e-3)
        else:
            SCG.close(p.grad.reshape(-1)[torch.from_numpy(idx).to(DEV)], z[pre + "grad." + k + "#sample"], "grad sample " + k, atol=2e-4, rtol=2e-3)
            want = float(z[pre + "grad." + k + "#norm"])
            assert abs(float(p.grad.double().norm()) - want) <= 2e-4 + 2e-3 * want, k
        seen += 1
    assert seen == sum(1 for k in z if k.startswith(pre + "grad.") and not k.endswith("#norm"))


# ------------------------------------------------------------------------------------------------------ 2. the pick changes no arithmetic
@pytest.mark.parametrize("name", SG.MODELS)
def test_free_running_step_equals_the_step_injected_with_its_own_tokens_bit_for_bit(golden, name):
    g = golden(name)
    m = SCG.build(g, g.group("weights"))
    batch = g.tensors("inputs")
    b5, T, n = batch["labels"].size(0), batch["labels"].size(1) - 2, 3
    rw = seeded_reward(b5, T, m.vocab_size)
    res = []
    with ops.deterministic():
        for calls in (0, 0, 1):
            torch.manual_seed(11)
            m.__dict__["_sample_calls"] = calls
            out, grads = step(m, batch, rw, IDX, n)
            res.append((m.sc_stats["seq"].clone(), out["lang_loss"].clone(), out["reward"].clone(), grads))
        out, grads = step(m, batch, rw, IDX, n, tokens=res[0][0])
    assert res[0][0].shape == (n * b5, T) and bool(res[0][0].any()) and abs(float(res[0][1])) > 0
    for a, b in zip(res[0], res[1]):                                             # two free runs from one seed
        assert torch.equal(a, b)
    assert not torch.equal(res[0][0], res[2][0])                                 # another call count: another stream
    assert torch.equal(out["lang_loss"], res[0][1]) and torch.equal(out["reward"], res[0][2]) and torch.equal(grads, res[0][3])
    assert float(grads.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------ 3. the draws
def test_every_draw_is_the_inverse_cdf_pick_on_the_logits_the_criterion_reads(golden):
    """Injected uniforms; the tap hands back every step's log-probabilities (the raw logits minus their row's lse: the same softmax).
    The method of test_rollout_greedy_half_..._inverse_cdf: every live draw is the fp64 inverse-CDF pick for its u; a draw whose u lies
    within 1e-5 of a CDF boundary is left out, at most 5 % of the live draws (expected share 2e-5 * 50 = 1e-3)."""
    g = golden("subgc_train")
    m = SCG.build(g, g.group("weights"))
    batch = g.tensors("inputs")
    b5, T, n = batch["labels"].size(0), batch["labels"].size(1) - 2, 3
    S = n * b5
    u = torch.rand(T, S, generator=torch.Generator().manual_seed(99)).to(DEV)
    m.tap = {}
    try:
        out, _ = step(m, batch, seeded_reward(b5, T, m.vocab_size), IDX, n, u=u)
        tap = m.tap
    finally:
        m.tap = None
    tok, lp, uu = host(m.sc_stats["seq"]), host(tap["step_logp"]).astype(np.float64), host(u)
    seqlp = host(m.sc_stats["seqlp"])
    assert tok.shape == (S, T) and lp.shape[:2] == (T + 1, S) and torch.isfinite(out["lang_loss"])
    assert np.array_equal(host(tap["fed_tokens"])[1:], tok.T) and not host(tap["fed_tokens"])[0].any()      # the words fed are the words drawn
    live = skipped = 0
    for r, t in live_steps(tok):
        live += 1
        assert abs(seqlp[r, t] - lp[t, r, tok[r, t]]) <= 1e-5, (r, t)
        if G.boundary_distance(lp[t, r], uu[t, r]) < 1e-5:
            skipped += 1
            continue
        assert tok[r, t] == G.inv_cdf_pick(lp[t, r], uu[t, r]), (r, t)
    for r in range(S):                                                           # a row is 0 from its end token on
        z = np.flatnonzero(tok[r] == 0)
        assert not len(z) or not tok[r, z[0]:].any()
    print(f"one-pass draws: {live} live, {skipped} skipped near a boundary, {int((tok > 0).sum())} words")
    assert live >= S and skipped <= 0.05 * live
    assert len({tuple(tok[k * b5:(k + 1) * b5].reshape(-1)) for k in range(n)}) == n      # the n sample blocks differ


# ------------------------------------------------------------------------------------------------------ 4. one pass = two passes
@pytest.mark.parametrize("name", SG.MODELS)
def test_one_pass_equals_the_two_pass_replay_of_its_tokens_with_its_rewards(golden, name):
    """n = 2.  The two-pass step differentiates its sampled half only, so the one-pass loss over both halves is the mask-weighted mean
    of two replays, (A; B) and (B; A), each made to use the rewards the one-pass step formed; so are the gradients."""
    g = golden(name)
    m = SCG.build(g, g.group("weights"))
    batch = g.tensors("inputs")
    b5, T = batch["labels"].size(0), batch["labels"].size(1) - 2
    rw = seeded_reward(b5, T, m.vocab_size)
    with ops.deterministic():
        torch.manual_seed(5)
        out, g1 = step(m, batch, rw, IDX, 2)
        seq, rewards = m.sc_stats["seq"].clone(), m.sc_stats["rewards"].clone()
        l1 = float(out["lang_loss"])
        tok = host(seq)
        halves = []
        for first in (0, 1):
            order = torch.cat([seq[first * b5:(first + 1) * b5], seq[(1 - first) * b5:(2 - first) * b5]]).contiguous()
            r_half = rewards[first * b5:(first + 1) * b5].contiguous()
            rw.enqueue = lambda seq2, d_index, rows=None, r_half=r_half: (r_half, r_half[:, 0].mean(), None)
            m.packed_decoder = False
            try:
                o2, g2 = step(m, batch, rw, IDX, 1, tokens=order)
            finally:
                del rw.enqueue
            den = float(G.mask_of(tok[first * b5:(first + 1) * b5]).sum())               # RewardCriterion's mask sum (the closing step has mask 0)
            halves.append((float(o2["lang_loss"]), g2.double(), den, float(o2["gpn_loss"]) if o2["gpn_loss"] is not None else 0.0))
    (la, ga, da, _), (lb, gb, db, _) = halves
    want_l = (la * da + lb * db) / (da + db)
    want_g = ((ga * da + gb * db) / (da + db)).float()
    print(f"{name}: one pass {l1:.8f} two passes {want_l:.8f} (dens {da:.0f} + {db:.0f})")
    assert abs(l1 - want_l) < 2e-5 * max(1.0, abs(l1)) and abs(l1) > 1e-4
    scale = float(want_g.abs().max())
    np.testing.assert_allclose(g1.cpu().numpy(), want_g.cpu().numpy(), atol=2e-5 * scale + 1e-7, rtol=2e-4)


# ------------------------------------------------------------------------------------------------------ 5. the reward
@pytest.mark.parametrize("n", SG.NS_CASE)
def test_device_reward_is_the_restatement_on_the_device_scores_bit_for_bit(n):
    z = SG.load("sc_samples_case.npz")
    refs = selfcritical.RewardReferences(G.per_image(z["ref_rows"], z["ref_cap_off"]))
    wc, wb = (float(x) for x in z["weights"])
    rw = selfcritical.SelfCriticalReward(refs, wc, wb)
    tok = z[f"n{n}.tok"]
    S, T = tok.shape
    d_index = dev(np.array([0, 1]), torch.int32)
    buf = dev(np.concatenate([tok, np.zeros_like(tok)]))
    _, _, rows = ops.sc_prepare(buf, refs.n_ids + 1, refs.eos_id, want_replay=False)
    reward, mean, scores, baseline = rw.enqueue_loo(rows, S, d_index, n)
    torch.cuda.synchronize()
    sc, r, b = host(scores), host(reward), host(baseline)
    assert r.shape == (S, T + 1) and r.dtype == np.float32 and (r == r[:, :1]).all() and sc.dtype == b.dtype == np.float64
    tol = wc * AG.CIDER_TOL * np.abs(z[f"n{n}.cider"]).max() + wb * AG.BLEU_TOL * np.abs(z[f"n{n}.bleu"][:, 3]).max() + 1e-16
    assert np.abs(sc - z[f"n{n}.scores"]).max() <= tol                          # the reference's scorers
    want_r, want_b, want_mean = selfcritical.loo_reward_restatement(sc, n)
    assert np.array_equal(r[:, 0], want_r) and np.array_equal(b, want_b)         # bit for bit
    assert abs(float(mean) - want_mean) <= U * np.abs(want_r).max() + S * SG.EPS * np.abs(want_r).max()
    assert np.abs(r[:, 0] - z[f"n{n}.reward"]).max() <= 4 * tol + U * np.abs(z[f"n{n}.reward"]).max()
    print(f"n={n}: score err {np.abs(sc - z[f'n{n}.scores']).max():.2e} reward err {np.abs(r[:, 0] - z[f'n{n}.reward']).max():.2e}")
    if n == 2:                                                                   # subgc_sc_reward itself on the same scored rows
        r2, _, s2 = rw.enqueue(dev(tok), d_index)
        assert np.array_equal(host(s2), sc)
        assert np.array_equal(host(r2), r[:S // 2]) and np.array_equal(-host(r2), r[S // 2:])


def test_word_gather_replicates_integer_rows_bit_for_bit():
    rep = dev(np.tile(np.arange(5), 3), torch.int32)
    for t in (torch.arange(5, dtype=torch.int32) * 7 - 3, torch.tensor([0, 1, -1, 2 ** 62 + 5, -2 ** 40]).view(5, 1).expand(5, 3).contiguous(),
              torch.tensor([0x7FC00001, 0x7F800001, 1, -1, 0x00400000], dtype=torch.int32)):
        got = ops.gather_rows_words(t.to(DEV), rep)
        assert got.dtype == t.dtype and torch.equal(got.cpu(), torch.cat([t, t, t]))


# ------------------------------------------------------------------------------------------------------ 6. bf16 storage
@pytest.mark.parametrize("packed", [True, False])
def test_bf16_storage_samples_from_its_own_logits_and_follows_the_fp32_step(golden, packed):
    g = golden("subgc_train")
    batch = g.tensors("inputs")
    b5, T, n = batch["labels"].size(0), batch["labels"].size(1) - 2, 2
    m = SCG.build(g, g.group("weights"), compute_dtype="bf16")
    assert m.bf16_storage
    m.packed_decoder = packed
    rw = seeded_reward(b5, T, m.vocab_size)
    u = torch.rand(T, n * b5, generator=torch.Generator().manual_seed(7)).to(DEV)
    out, grads = step(m, batch, rw, IDX, n, u=u)
    tok, seqlp = host(m.sc_stats["seq"]), host(m.sc_stats["seqlp"])
    assert torch.isfinite(out["lang_loss"]) and bool(torch.isfinite(grads).all()) and float(grads.abs().max()) > 0
    ref = SCG.build(g, g.group("weights"))
    ref.packed_decoder = packed
    ref.tap = {}
    try:
        out32, _ = step(ref, batch, rw, IDX, n, tokens=tok)
        lp32 = host(ref.tap["step_logp"])
    finally:
        ref.tap = None
    worst = max(abs(float(seqlp[r, t]) - float(lp32[t, r, tok[r, t]])) for r, t in live_steps(tok))
    print(f"packed={packed}: bf16 loss {float(out['lang_loss']):.6f} fp32 {float(out32['lang_loss']):.6f}, worst |seqlp - fp32| {worst:.2e}")
    assert worst <= 5e-2
    assert float(out["reward"]) == float(out32["reward"])                       # fp64 scores of the same tokens
    assert abs(float(out["lang_loss"]) - float(out32["lang_loss"])) <= 5e-2 and float(out["lang_loss"]) != float(out32["lang_loss"])


# ------------------------------------------------------------------------------------------------------ 7. sc_samples = 1 is today's step
class _Opt:
    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.mark.parametrize("name", SG.MODELS)
def test_one_sample_and_no_option_are_the_two_pass_step_and_sc_flag_false_is_untouched(golden, name):
    g = golden(name)
    m = SCG.build(g, g.group("weights"))
    batch = g.tensors("inputs")
    b5, T = batch["labels"].size(0), batch["labels"].size(1) - 2
    rw = seeded_reward(b5, T, m.vocab_size)
    res, plain = [], []
    with ops.deterministic():
        for kw in ({"n": None}, {"n": 1}, {"n": None, "opt": _Opt(train_sample_n=1)}, {"n": None, "opt": _Opt()}):
            torch.manual_seed(11)
            m.__dict__["_sample_calls"] = 0
            out, grads = step(m, batch, rw, IDX, **kw)
            assert m.sc_stats["seq"].shape == (2 * b5, T) and set(m.sc_stats) == {"reward", "seq"}      # rollout + replay, greedy half
            res.append((out["lang_loss"].clone(), out["reward"].clone(), m.sc_stats["seq"].clone(), grads))
        for n in (None, 3):
            m._dropout_calls = 0
            out, grads = step(m, batch, rw, IDX, n, sc_flag=False)
            assert set(out) == {"gpn_loss", "lang_loss"}
            plain.append((out["lang_loss"].clone(), grads))
    for other in res[1:]:
        assert all(torch.equal(a, b) for a, b in zip(res[0], other))
    assert torch.equal(plain[0][0], plain[1][0]) and torch.equal(plain[0][1], plain[1][1])
    SCG.close(plain[0][0], g.group("out")["lang_loss"], "lang_loss", atol=1e-4, rtol=1e-4)


# ------------------------------------------------------------------------------------------------------ 8. bounds and poison
def _poison(monkeypatch):
    """tests/conftest.py's SUBGC_POISON_EMPTY rule for the length of one test: every buffer torch.empty hands out starts as NaN / a large
    integer, so a kernel that reads what nobody wrote changes the result."""
    def poisoned(fn):
        def wrap(*a, **k):
            t = fn(*a, **k)
            if t.is_cuda and t.numel():
                t.fill_(float("nan")) if t.is_floating_point() else (t.fill_(0x3fffffff) if t.dtype in (torch.int32, torch.int64) else t.fill_(255))
            return t
        return wrap
    monkeypatch.setattr(torch, "empty", poisoned(torch.empty))
    monkeypatch.setattr(torch, "empty_like", poisoned(torch.empty_like))


@pytest.mark.parametrize("mode", ["debug_bounds", "poison"])
def test_free_running_step_under_debug_bounds_and_with_poisoned_buffers(golden, monkeypatch, mode):
    g = golden("subgc_train")
    m = SCG.build(g, g.group("weights"))
    batch = g.tensors("inputs")
    b5, T, n = batch["labels"].size(0), batch["labels"].size(1) - 2, 3
    rw = seeded_reward(b5, T, m.vocab_size)
    with ops.deterministic():
        torch.manual_seed(3)
        m.__dict__["_sample_calls"] = 0
        want, want_g = step(m, batch, rw, IDX, n)
        want_seq = m.sc_stats["seq"].clone()
        torch.manual_seed(3)
        m.__dict__["_sample_calls"] = 0
        if mode == "poison":
            _poison(monkeypatch)
            out, grads = step(m, batch, rw, IDX, n)
            monkeypatch.undo()
        else:
            with ops.debug_bounds():
                out, grads = step(m, batch, rw, IDX, n)
    seq = m.sc_stats["seq"]
    assert seq.shape == (n * b5, T) and int(seq.min()) >= 0 and int(seq.max()) <= m.vocab_size and torch.equal(seq, want_seq)
    assert torch.isfinite(out["lang_loss"]) and torch.isfinite(out["reward"]) and bool(torch.isfinite(grads).all())
    assert torch.equal(out["lang_loss"], want["lang_loss"]) and torch.equal(grads, want_g)
