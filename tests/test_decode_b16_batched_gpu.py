"""The opt-in bf16-batched decode regime (opt.decode_b16_batched; functions.DecodeState of more than 32 rows under compute_dtype = bf16) on
the MI355X: the two kernels of include/subgc_decode_b16_hip.h against the numpy restatement (decode_b16_restatement.py), two steps of the
state stage by stage from the operands the device itself used, and the model paths -- image batch, top-k, forced decode, beam / diverse
beam search, the self-critical rollout -- against the fp32 oracle at SURVEY 8(c)'s bf16 tolerance.

Input choice (test_decode_b16_cpu.py, no GPU): on the 40-row batch used here -- images (0, 2, 3, 6) of
test_bf16_sample_images_batches_in_each_row_regime -- the restated regime stays within 1.273e-02 of the fp32 oracle's log-probs on every
live step of the oracle's own greedy captions (tolerance 5e-2).

Tolerances, all taken from existing tests:
  cell state c     atol 1e-6, rtol 1e-4    tests/test_kernels_gpu.py:296 (subgc_lstm_fwd's c; `close` defaults to rtol 1e-4, :19)
  bf16 h           within ONE bf16 spacing of bf16(h restated): fp32 values that close round to equal or neighbouring bf16 values
  products         max |got - fp64| < 2e-5 * max |fp64| on the same bf16 operands    tests/test_gemm_bf16_gpu.py:39
  attention        alpha atol 1e-5 (tests/test_decode_bf16_gpu.py:189); ctx: one bf16 rounding of the fp64 value plus that fp32 tolerance
                   carried through the convex combination, 2^-8 |ctx| + 1e-5 max |v|
  model level      log-probs 5e-2, attention 2e-2 (test_decode_bf16_gpu._same_path_as_oracle)"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import decode_b16_restatement as RS
import self_critical_golden as SG
from oracle import subgc_oracle as O
from subgc import beam, forced, functions as F_, ops, selfcritical, synthetic
from subgc.models import sampling
from test_decode_b16_cpu import TOPK_SEED, batch_images, explain_forks
from test_decode_bf16_gpu import _same_path_as_oracle, _upto_eos, states  # noqa: F401  (`states` is a fixture)
from test_parity_gpu import DEV, build, close

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def host64(t):
    return t.detach().double().cpu().numpy()


def ordered(bits):
    """bf16 bit patterns -> integers in value order (neighbouring values differ by 1, +0 and -0 coincide)."""
    b = np.asarray(bits).astype(np.int64)
    return np.where(b & 0x8000, -(b & 0x7FFF), b & 0x7FFF)


def bits_of(t):
    return t.contiguous().view(torch.int16).cpu().numpy().astype(np.int64) & 0xFFFF


def spacing_apart(h_dev, h_ref64):
    """-> (largest distance in bf16 spacings between the device's bf16 h and bf16(h restated), share of elements that differ at all)."""
    d = np.abs(ordered(bits_of(h_dev)) - ordered(RS.bf16_bits(h_ref64)))
    return int(d.max()), float((d > 0).mean())


def check_c(c_dev, c_ref, what):
    np.testing.assert_allclose(host64(c_dev), c_ref, atol=1e-6, rtol=1e-4, err_msg=what)


def check_product(got, ref, what):
    err, scale = float(np.abs(host64(got) - ref).max()), float(np.abs(ref).max())
    assert err < 2e-5 * scale, (what, err, scale)


# ------------------------------------------------------------------------------------------------------------------ 1. the cell
def _well_conditioned(c_of, x, floor=1e-3):
    """Input choice, made on the host from the restatement alone before anything runs on the device: `x` (c_prev, or the g-gate
    pre-activations when there is no c_prev) is moved by 0.25 wherever the restated |c| = |c_of(x)| is below `floor`.  c is a sum of two
    products of order 0.3, so its fp32 value carries an ABSOLUTE error of a few 1e-8 (well inside the c tolerance); h = o tanh(c)
    inherits that error relatively, and below |c| ~ 1e-5 it exceeds a bf16 spacing (2^-8 |h|): there "within one bf16 spacing" asks
    more than fp32 arithmetic gives.  The bound itself stays as it is."""
    x = x.clone()
    for _ in range(8):
        small = torch.from_numpy(np.abs(c_of(x)) < floor).to(x.device)
        if not bool(small.any()):
            return x
        x[small] += 0.25
    raise AssertionError("could not move the cell state away from zero")


@pytest.mark.parametrize("R", [8, 48, 1000])
@pytest.mark.parametrize("S", [1, 33, 130])
def test_cell_equals_the_restatement(S, R):
    """subgc_decode_cell_b16: with / without the x->gates table and g2, two and three destinations with distinct pitches inside sentinel-
    filled buffers, tokens 0, vocab_rows - 1, -1 and one past the table."""
    V = 23
    g = torch.Generator().manual_seed(1000 * S + R)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(DEV)
    table, b0, b1 = rnd(V, 4 * R, sc=0.5), rnd(4 * R, sc=0.3), rnd(4 * R, sc=0.3)
    special = [0, V - 1, -1, V]
    for case, (use_table, use_g2, n_dst) in enumerate([(True, True, 2), (True, False, 3), (False, True, 3), (False, False, 2)]):
        pre_buf = rnd(S, 4 * R + 4)
        g0, g2, cp = pre_buf[:, :4 * R], rnd(S, 4 * R, sc=0.5), rnd(S, R)
        tok = torch.randint(-1, V + 2, (S,), generator=g)
        tok[:min(S, 4)] = torch.tensor((special[case:] + special[:case])[:min(S, 4)])
        tok = tok.to(DEV)
        args64 = (host64(g0), host64(table) if use_table else None, tok.cpu().numpy(), host64(g2) if use_g2 else None,
                  host64(b0) if case != 3 else None, host64(b1))
        cp = _well_conditioned(lambda x: RS.cell(RS.cell_pre(*args64), host64(x))[0], cp)
        c = torch.full((S, R), 5.0, device=DEV)
        bufs =[torch.full((S, 3 * R), 9.0, device=DEV, dtype=BF), torch.full((S + 1, R + 24), 9.0, device=DEV, dtype=BF),
                torch.full((S, R + 64), 9.0, device=DEV, dtype=BF)]
        hs = [bufs[0][:, R:2 * R], bufs[1][:S, 8:8 + R], bufs[2][:, :R]][:n_dst]
        assert len({ops.ld(h) for h in hs}) == n_dst
        ops.decode_cell_b16(g0, cp, c, hs, b0 if case != 3 else None, b1, table if use_table else None, tok if use_table else None,
                            g2 if use_g2 else None)
        c_ref, h_ref = RS.cell(RS.cell_pre(*args64), host64(cp))
        check_c(c, c_ref, f"c case {case}")
        far, share = spacing_apart(hs[0], h_ref)
        print(f"S={S} R={R} case {case}: bf16 h differs from bf16(restated) in {share:.2e} of the elements, at most {far} spacing(s)")
        assert far <= 1
        assert all(torch.equal(h, hs[0]) for h in hs[1:])
        nine = lambda t: t.numel() == 0 or (float(t.float().min()) == 9.0 and float(t.float().max()) == 9.0)
        assert nine(bufs[0][:, :R]) and nine(bufs[0][:, 2 * R:]) and nine(bufs[1][S]) and nine(bufs[1][:, :8]) and nine(bufs[1][:, 8 + R:])
        assert nine(bufs[2][:, R:])
        if n_dst == 2:
            assert nine(bufs[2])
    c2, h2 = torch.empty(S, R, device=DEV), torch.empty(S, R, device=DEV, dtype=BF)                 # no c_prev, nothing additive
    g0 = g0.contiguous()
    g0[:, 2 * R:3 * R] = _well_conditioned(lambda x: RS.cell(np.concatenate([host64(g0[:, :2 * R]), host64(x), host64(g0[:, 3 * R:])], 1), None)[0],
                                           g0[:, 2 * R:3 * R].contiguous())
    ops.decode_cell_b16(g0, None, c2, [h2])
    c_ref, h_ref = RS.cell(host64(g0), None)
    check_c(c2, c_ref, "c without c_prev")
    assert spacing_apart(h2, h_ref)[0] <= 1


# ------------------------------------------------------------------------------------------------------------------ 2. the fork
@pytest.mark.parametrize("R", [8, 48])
@pytest.mark.parametrize("S", [1, 33, 130])
def test_fork_equals_the_numpy_gather(S, R):
    """subgc_decode_fork_b16 on the layout DecodeState.reorder hands it: H1 whole, the h_lang slot of H2, c1, c2, every buffer with padding."""
    g = torch.Generator().manual_seed(7 * S + R)
    rb = lambda r, c: torch.randn(r, c, generator=g).to(DEV).to(BF)
    rf = lambda r, c: torch.randn(r, c, generator=g).to(DEV)
    perm = torch.randperm(S, generator=g)
    for kind, src in (("identity", torch.arange(S)), ("permutation", perm), ("fork", perm[torch.randint(0, max(S // 3, 1), (S,), generator=g)])):
        H1, H2, c1, c2 = rb(S, 2 * R + 8), rb(S, 3 * R + 64), rf(S, R), rf(S, R + 4)
        before = [t.clone() for t in (H1, H2, c1, c2)]
        d1 = torch.full((S, 2 * R + 16), 9.0, device=DEV, dtype=BF)
        d2 = torch.full((S, 3 * R + 8), 9.0, device=DEV, dtype=BF)
        dc1, dc2 = torch.full((S, R + 8), 9.0, device=DEV), torch.full((S, R), 9.0, device=DEV)
        idx = src.to(torch.int32).to(DEV)
        ops.decode_fork_b16([(H1[:, :2 * R], d1[:, :2 * R]), (H2[:, 2 * R:3 * R], d2[:, 2 * R:3 * R])], [(c1, dc1[:, :R]), (c2[:, :R], dc2)], idx)
        s = src.numpy()
        for got, want in ((d1[:, :2 * R], H1[:, :2 * R]), (d2[:, 2 * R:3 * R], H2[:, 2 * R:3 * R]), (dc1[:, :R], c1), (dc2, c2[:, :R])):
            a = got.contiguous().view(torch.int16 if got.dtype == BF else torch.int32).cpu().numpy()
            b = want.contiguous().view(torch.int16 if got.dtype == BF else torch.int32).cpu().numpy()
            np.testing.assert_array_equal(a, b[s], err_msg=kind)
        for t, t0 in zip((H1, H2, c1, c2), before):                                                       # the sources are unchanged
            assert torch.equal(t, t0), kind
        for pad in (d1[:, 2 * R:], d2[:, :2 * R], d2[:, 3 * R:], dc1[:, R:]):                             # and so is the padding
            assert float(pad.float().min()) == 9.0 and float(pad.float().max()) == 9.0, kind


def test_fork_clamps_rows_outside_the_state():
    S, R = 5, 8
    H1 = torch.arange(S, device=DEV).view(S, 1).expand(S, 2 * R).to(BF).contiguous()
    H2 = H1[:, :R].contiguous()
    c1 = torch.arange(S, device=DEV).float().view(S, 1).expand(S, R).contiguous()
    out = [torch.empty_like(t) for t in (H1, H2, c1, c1)]
    src = torch.tensor([-3, 0, 4, 5, 99], dtype=torch.int32, device=DEV)
    ops.decode_fork_b16([(H1, out[0]), (H2, out[1])], [(c1, out[2]), (c1, out[3])], src)
    for o in out:
        assert o[:, 0].float().cpu().tolist() == [0.0, 0.0, 4.0, 4.0, 4.0]


# ------------------------------------------------------------------------------------------------------------------ 3. two steps, stage by stage
def _golden_model(golden, name="subgc_greedy", **over):
    g = golden(name)
    w = golden("subgc_train").group("weights")
    return g, w, build(g, w, False, compute_dtype="bf16", **over)


@pytest.mark.parametrize("S", [40, 130])
def test_two_steps_of_the_state_stage_by_stage(golden, monkeypatch, S):
    """Every stage of two bf16-batched steps recomputed in fp64 from the operands the device itself used (its bf16 state buffers, its fp32
    pre-activations and table) and the MODEL's own twins: pre1, cell, ah, ctx, pre2, cell, logits.  S = 130: a partial second 128-row tile."""
    g, w, m = _golden_model(golden, decode_b16_batched=1)
    R, V1 = m.rnn_size, m.vocab_size + 1
    gen = torch.Generator().manual_seed(60 + S)
    Nn = 7
    fc = torch.randn(S, m.P("fc_embed.0.weight").size(1), generator=gen)
    att = torch.randn(S, Nn, m.P("att_embed.0.weight").size(1), generator=gen)
    lens = torch.randint(1, Nn + 1, (S,), generator=gen)
    lens[0] = Nn
    masks = (torch.arange(Nn).view(1, Nn) < lens.view(-1, 1)).float()
    p_fc, p_att, pp_att, p_masks = m._prepare_feature(fc.to(DEV), att.to(DEV), masks.to(DEV))
    n_max = p_att.size(1)
    pr = SimpleNamespace(S=S, N=n_max, f=p_fc.contiguous(), u=pp_att.contiguous().view(S * n_max, -1), v=p_att.contiguous().view(S * n_max, R),
                         off=(torch.arange(S, device=DEV, dtype=torch.int32) * n_max).contiguous(), lens=p_masks.sum(1).to(torch.int32).contiguous())
    st = F_.DecodeState(pr, m._decoder_params(), n_max, True, xt_table=m.xt_gates_table(), fuse_lstm=True, snapshots=m.decode_snapshots(),
                        W16=m.decode_w16(), b16_batched=True)
    assert st.regime == "bf16-batched" and not st.fused and "cat16" in m.decode_snapshots() and "perm16" not in m.decode_snapshots()
    assert st.H1.dtype == BF and st.H2.dtype == BF and st.hout.dtype == BF and st.C1[0].dtype == torch.float32
    assert ops.ld(st.H1) % 8 == 0 and ops.ld(st.H2) % 8 == 0 and ops.ld(st.hout) % 8 == 0
    twin = lambda k: host64(m.W16(k, m.weights_b16()))
    Wc1 = np.concatenate([twin("core.att_lstm.weight_ih")[:, :R], twin("core.att_lstm.weight_hh")], 1)
    Wc2 = np.concatenate([twin("core.lang_lstm.weight_ih"), twin("core.lang_lstm.weight_hh")], 1)
    h2a, lg = twin("core.attention.h2att.weight"), twin("logit.weight")
    p64 = lambda k: host64(m.P(k))
    check_product(st.Gf, RS.bf16(host64(p_fc)) @ twin("core.att_lstm.weight_ih")[:, R:2 * R].T, "Gf")
    st.H1.copy_((torch.randn(S, 2 * R, generator=gen) * 0.3).to(DEV))                 # a state that is not zero: [h_lang | h_att]
    st.H2[:, 2 * R:].copy_(st.H1[:, :R])
    st.C1[0].copy_((torch.randn(S, R, generator=gen) * 0.3).to(DEV)); st.C2[0].copy_((torch.randn(S, R, generator=gen) * 0.3).to(DEV))
    seen = {"cell": [], "attn": []}
    real_cell, real_attn = ops.decode_cell_b16, ops.attn_fwd

    def spy_cell(g0, c_prev, c, hs, *a, **k):
        rec = dict(pre=g0.clone(), c_prev=c_prev.clone())
        real_cell(g0, c_prev, c, hs, *a, **k)
        rec.update(c=c.clone(), h=[h.clone() for h in hs])
        seen["cell"].append(rec)

    def spy_attn(u, v, ah, *a, **k):
        seen["attn"].append(ah.clone())
        real_attn(u, v, ah, *a, **k)

    monkeypatch.setattr(ops, "decode_cell_b16", spy_cell)
    monkeypatch.setattr(ops, "attn_fwd", spy_attn)
    table = host64(st.xt_table)
    u3, v3, mk = host64(pp_att), host64(p_att), host64(p_masks)
    toks = torch.randint(0, V1, (2, S), generator=gen)
    alpha = torch.zeros(S, n_max, device=DEV)
    for t in range(2):
        H1_in, hl_in = host64(st.H1), host64(st.H2[:, 2 * R:])
        del seen["cell"][:], seen["attn"][:]
        logits = st.step(toks[t].to(DEV), alpha, normalize=False)
        c1r, c2r = seen["cell"]
        check_product(c1r["pre"], H1_in @ Wc1.T, f"pre1 step {t}")
        pre = RS.cell_pre(host64(c1r["pre"]), table, toks[t].numpy(), host64(st.Gf), p64("core.att_lstm.bias_ih"), p64("core.att_lstm.bias_hh"))
        c_ref, h_ref = RS.cell(pre, host64(c1r["c_prev"]))
        check_c(c1r["c"], c_ref, f"c_att step {t}")
        assert spacing_apart(c1r["h"][0], h_ref)[0] <= 1 and torch.equal(c1r["h"][0], c1r["h"][1])
        assert torch.equal(st.H2[:, R:2 * R], c1r["h"][0]) and torch.equal(st.H1[:, R:], c1r["h"][0]) and torch.equal(st.C1[0], c1r["c"])
        h_att = host64(c1r["h"][0])
        check_product(seen["attn"][0], h_att @ h2a.T + p64("core.attention.h2att.bias"), f"ah step {t}")
        ctx_ref, a_ref = RS.attention(host64(seen["attn"][0]), u3, v3, mk, p64("core.attention.alpha_net.weight"), p64("core.attention.alpha_net.bias"))
        np.testing.assert_allclose(host64(alpha), a_ref, atol=1e-5, rtol=1e-5, err_msg=f"alpha step {t}")
        ctx = host64(st.H2[:, :R])
        assert float((np.abs(ctx - ctx_ref) - 2.0 ** -8 * np.abs(ctx_ref)).max()) <= 1e-5 * float(np.abs(v3).max()), f"ctx step {t}"
        check_product(c2r["pre"], np.concatenate([ctx, h_att, hl_in], 1) @ Wc2.T, f"pre2 step {t}")
        pre = RS.cell_pre(host64(c2r["pre"]), b0=p64("core.lang_lstm.bias_ih"), b1=p64("core.lang_lstm.bias_hh"))
        c_ref, h_ref = RS.cell(pre, host64(c2r["c_prev"]))
        check_c(c2r["c"], c_ref, f"c_lang step {t}")
        assert spacing_apart(c2r["h"][0], h_ref)[0] <= 1 and all(torch.equal(h, c2r["h"][0]) for h in c2r["h"][1:]) and len(c2r["h"]) == 3
        assert torch.equal(st.H1[:, :R], c2r["h"][0]) and torch.equal(st.H2[:, 2 * R:], c2r["h"][0]) and torch.equal(st.hout, c2r["h"][0])
        check_product(logits, host64(st.hout) @ lg.T + p64("logit.bias"), f"logits step {t}")
    # the product check tells the twins from the fp32 masters: the same stage on the fp32 logit matrix misses the tolerance
    far = np.abs(host64(logits) - (host64(st.hout) @ p64("logit.weight").T + p64("logit.bias"))).max()
    assert far > 2e-5 * np.abs(host64(logits)).max()
    # a missing twin leaves the fp32 regime, and so does a state built without the keyword; `regime` says so
    W16 = list(m.decode_w16()); W16[17] = None
    assert F_.DecodeState(pr, m._decoder_params(), n_max, False, xt_table=m.xt_gates_table(), fuse_lstm=True, W16=W16, b16_batched=True).regime == "fp32"
    assert F_.DecodeState(pr, m._decoder_params(), n_max, False, xt_table=m.xt_gates_table(), fuse_lstm=True, W16=m.decode_w16()).regime == "fp32"


# ------------------------------------------------------------------------------------------------------------------ 4. model level
def _on_device(ims):
    return [{k: v.to(DEV) for k, v in b.items()} for b in ims]


def test_sample_images_forced_decode_and_attention_follow_the_oracle(golden, states):
    g, w, m = _golden_model(golden, decode_b16_batched=1)
    ims = batch_images(g)
    orc = O.Oracle(g.opt(), w)
    greedy = None
    for return_att in (0, 1):
        del states[:]
        sopt = dict(sample_max=1, beam_size=1, return_att=return_att)
        out = m.sample_images(_on_device(ims), opt=sopt)
        assert sum(r[0].size(0) for r in out) == 40
        assert [st.S for st in states] == [40] and states[0].regime == "bf16-batched"
        for r, b in zip(out, ims):
            assert len(r) == 4 + return_att
            _same_path_as_oracle(r, orc, b, sopt, min_same=r[0].size(0) // 2)
        greedy = greedy or out
    for a, b in zip(greedy, out):                                                   # return_att changes no token
        assert torch.equal(a[0], b[0])
    # forced decode along the greedy tokens: candidate keep[j] of an image follows its row j
    del states[:]
    toks = []
    for r, b in zip(greedy, ims):
        tok = np.zeros((int(b["gpn_obj_ind"].size(1) * b["gpn_obj_ind"].size(2)), m.seq_length), np.int64)
        tok[r[3].cpu().numpy().astype(np.int64)] = r[0].cpu().numpy()
        toks.append(tok)
    f = forced.forced_decode(m, _on_device(ims), toks)
    assert len(states) == 1 and states[0].S == f["rows"] > 40 and states[0].regime == "bf16-batched"
    worst = 0.0
    for r, a in zip(greedy, f["bounds"]):
        where = (a + r[3].cpu().numpy().astype(np.int64)).tolist()
        seq, live = r[0].cpu(), _upto_eos(r[0].cpu())
        assert torch.equal(f["seq"][where].cpu() * live, seq * live)
        worst = max(worst, float((f["seqlp"][where].cpu() - r[1].cpu())[live].abs().max()))
    print(f"forced decode along the greedy tokens: max |d log-prob| on live steps = {worst:.3e}")
    assert worst <= 2e-5


def test_topk_sampling_with_injected_uniforms_follows_the_oracle(golden, states):
    """The 40-row batch with top-k sampling from injected uniforms; forks explained by
    test_bf16_topk_sampling_with_injected_uniforms_follows_the_oracle's rule."""
    g, w, m = _golden_model(golden, "subgc_topk", decode_b16_batched=1)
    sopt = g.meta["sample_opt"]
    ims = batch_images(golden("subgc_greedy"))
    dims = _on_device(ims)
    att, obj, pred, rel = ops.stack_first([[im[k] for im in dims] for k in ("att_feats", "obj_dist", "pred_dist", "rel_ind")])
    I, N, _ = att.shape
    with torch.no_grad():
        X2 = m._encode(att, obj, pred, rel).reshape(I * N, m.GCN_dim).contiguous()
        sel = sampling.select_subgraphs(m, X2, N, [(i, im["gpn_obj_ind"], im["att_masks"], im["gpn_pool_mtx"]) for i, im in enumerate(dims)])
        u = torch.rand(40, m.seq_length, generator=torch.Generator().manual_seed(TOPK_SEED))
        out = sampling.decode(m, X2, N, sel, sopt, uniforms=u.to(DEV))
    assert [st.S for st in states] == [40] and states[0].regime == "bf16-batched"
    orc = O.Oracle(g.opt(), w)
    a = 0
    for ret, b in zip(out, ims):
        n = ret[0].size(0)
        ub = u[a:a + n]
        a += n
        tap = {}
        want = orc.sample(*synthetic.sample_args(b), opt=sopt, uniforms=ub, tap=tap)
        fr = orc.sample(*synthetic.sample_args(b), opt=sopt, forced=ret[0].cpu())
        np.testing.assert_array_equal(ret[3].cpu().numpy(), want[3].numpy())
        got = ret[0].cpu()
        live = _upto_eos(got)
        close(ret[1].cpu()[live], fr[1][live], "topk seqLogprobs vs oracle", atol=5e-2, rtol=0)
        assert explain_forks(got, want[0], tap, ub, m.topk_temp) <= n - n // 2
    assert a == 40


# ------------------------------------------------------------------------------------------------------------------ 5. beam
def _beam_lens(seq):
    """Words of a beam, its end token counted; T for a beam cut at the last step."""
    z = (seq == 0)
    return torch.where(z.any(1), z.float().argmax(1) + 1, torch.full((seq.size(0),), seq.size(1), dtype=torch.long)).numpy()


@pytest.mark.parametrize("bopt", [dict(beam_size=2), dict(beam_size=4, group_size=2)])
def test_beam_search_on_the_batch_follows_the_oracle_and_forced_decode(golden, states, bopt):
    g, w, m = _golden_model(golden, decode_b16_batched=1)
    ims = batch_images(g)
    dims = _on_device(ims)
    sopt = dict(sample_max=1, return_att=1, **bopt)
    out = m.sample_images(dims, opt=sopt)
    assert [st.S for st in states] == [40 * bopt["beam_size"]] and all(st.regime == "bf16-batched" for st in states)
    assert not [k for k in m.__dict__.get("_graph_cache", {}) if k[0] == "beam"]                     # > 32 rows: eager
    bd = bopt["beam_size"] // bopt.get("group_size", 1)
    assert len(m.done_beams) == len(ims)
    for beams in m.done_beams:
        for row in beams:
            assert len(row) == bopt["beam_size"]
            for gi in range(bopt.get("group_size", 1)):
                ps = [b_["p"] for b_ in row[gi * bd:(gi + 1) * bd]]
                assert len(ps) == bd and ps == sorted(ps, reverse=True)
    orc = O.Oracle(g.opt(), w)
    toks = []
    for r, b in zip(out, ims):
        seq = r[0].cpu()
        fr = orc.sample(*synthetic.sample_args(b), opt=dict(sample_max=1, beam_size=1), forced=seq)
        np.testing.assert_array_equal(r[3].cpu().numpy(), fr[3].numpy())
        live = _upto_eos(seq)
        close(r[1].cpu()[live], fr[1][live], "beam seqLogprobs vs oracle", atol=5e-2, rtol=0)
        tok = np.zeros((int(b["gpn_obj_ind"].size(1) * b["gpn_obj_ind"].size(2)), m.seq_length), np.int64)
        tok[r[3].cpu().numpy().astype(np.int64)] = seq.numpy()
        toks.append(tok)
    # the gathered attention against a forced decode along the winners: the same regime on the same tokens
    f = forced.forced_decode(m, dims, toks, return_att=True)
    assert states[-1].regime == "bf16-batched"
    fa = f["AL"].cpu().numpy()
    worst = 0.0
    for r, a in zip(out, f["bounds"]):
        where = a + r[3].cpu().numpy().astype(np.int64)
        lens = _beam_lens(r[0].cpu())
        att = r[4].cpu().numpy()                                                                     # [rows, steps, n_max]
        steps, n_max = att.shape[1], att.shape[2]
        assert steps == int(lens.max())
        live = np.arange(steps)[None, :] < lens[:, None]
        worst = max(worst, float(np.abs(fa[:steps, where, :n_max].transpose(1, 0, 2) - att)[live].max()))
    print(f"{bopt}: beam attention against forced decode, max |d| = {worst:.3e}")
    assert worst <= 1e-5


def test_one_image_beam_with_the_option_on_takes_the_fused_regimes_and_a_graph(golden, states):
    """10 sub-graphs x beam 2 = 20 rows with the option on: the twins reach the engine, the state is the fused lstm-bf16 one, the search is
    captured, and the replayed search equals its eager run bit for bit."""
    g, w, m = _golden_model(golden, decode_b16_batched=1)
    tb = {k: v.to(DEV) for k, v in g.tensors("inputs").items()}
    sopt = dict(sample_max=1, beam_size=2)
    run = lambda mm: mm(*synthetic.sample_args(tb), opt=sopt, mode="sample")
    graphed = run(m)
    keys = [k for k in m._graph_cache if k[0] == "beam"]
    assert len(keys) == 1 and dict(keys[0][3])["b16_batched"] is True
    assert states and all(st.S == 20 and st.regime == "lstm-bf16" for st in states)
    again = run(m)
    _, _, e = _golden_model(golden, decode_b16_batched=1)
    e.decode_hipgraph = False
    eager = run(e)
    assert states[-1].regime == "lstm-bf16" and "_graph_cache" not in e.__dict__
    for r in (again, eager):
        assert torch.equal(r[0], graphed[0]) and torch.equal(r[1].view(torch.int32), graphed[1].view(torch.int32)) and torch.equal(r[3], graphed[3])


# ------------------------------------------------------------------------------------------------------------------ 6. the SCST rollout
def test_rollout_with_the_option_on(golden, monkeypatch, states):
    """The self-critical rollout of the subgc_train golden batch taken twice (6 images, 30 sub-graphs, 60 doubled rows) under bf16 storage
    with the option on.  (a) The greedy half equals a plain batched greedy decode of the same rows bit for bit.  (b) The sampled half: its
    own tokens forced through the same state give every step's row, and each live draw is the fp64 inverse-CDF pick for its u; a draw whose
    u lies within 1e-5 of a CDF boundary may be skipped, at most 1 % of the live draws (test_self_critical_gpu's rule)."""
    from test_self_critical_gpu import build as build_train, fixture_reward, pick_state, run_sc
    g, z = golden("subgc_train"), SG.load_train()
    m = build_train(g, g.group("weights"), compute_dtype="bf16", decode_b16_batched=1)
    T, b5 = 16, 30
    u = torch.rand(T, b5, generator=torch.Generator().manual_seed(99)).to(DEV)
    seen = {}
    real = selfcritical.rollout

    def spy(model, fc, Xb, lens, sel_idx, img_s, N, uniforms=None, T=None):
        seen.update(fc=fc.detach().clone(), Xb=Xb.detach().clone(), lens=lens.clone(), sel_idx=sel_idx.clone(), img_s=img_s.clone(), N=N)
        seen["seq2"] = real(model, fc, Xb, lens, sel_idx, img_s, N, uniforms=u, T=T)
        return seen["seq2"]

    monkeypatch.setattr(selfcritical, "rollout", spy)
    batch = {k: torch.cat([v, v]) for k, v in g.tensors("inputs").items()}
    gi = np.asarray(z["sc.gt_indices"])
    out = run_sc(m, batch, fixture_reward(z), np.concatenate([gi, gi]))
    seq2 = seen["seq2"]
    assert seq2.shape == (2 * b5, T) and torch.isfinite(out["lang_loss"]) and int(seq2.max()) <= m.vocab_size
    assert [st.S for st in states] == [2 * b5] and states[0].regime == "bf16-batched"
    two = lambda t: torch.cat([t, t]).contiguous()
    P = [p.detach() for p in m._decoder_params()]
    with torch.no_grad():
        pr = F_.Prepared(two(seen["fc"]), seen["Xb"], two(seen["lens"]), two(seen["sel_idx"]), two(seen["img_s"]), seen["N"], P, None, None, 1.0)
        st = F_.DecodeState(pr, P, seen["N"], False, xt_table=m.xt_gates_table(), fuse_lstm=True, snapshots=m.decode_snapshots(), W16=m.decode_w16(),
                            b16_batched=True)
        assert st.regime == "bf16-batched"
        s, l, it, unf, cnt = pick_state(2 * b5, T)
        for t in range(T):
            logits = st.step(it, None, normalize=False)
            ops.decode_pick(logits, 0, 1.0, None, t, s, l, it, unf, cnt[t:t + 1], cnt[t - 1:t] if t > 0 else None, raw=True)
        assert torch.equal(s[b5:], seq2[b5:]) and torch.equal(s[:b5], s[b5:]) and bool(s.any())
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
            if SG.boundary_distance(rows[t][sidx], uu[t, sidx]) < 1e-5:
                skipped += 1
                continue
            assert tok[sidx, t] == SG.inv_cdf_pick(rows[t][sidx], uu[t, sidx]), (sidx, t)
    print(f"rollout (bf16-batched): {live} live draws, {skipped} skipped near a boundary")
    assert live >= b5 and skipped <= 0.01 * live
    assert not torch.equal(seq2[:b5], seq2[b5:])


# ------------------------------------------------------------------------------------------------------------------ 7. option off
def test_option_off_is_the_fp32_regime_bit_for_bit(golden, states):
    """decode_b16_batched = 0 on a bf16 model: the 40-row batch and its beam-2 search run the fp32 regime and give the bits of a model built
    without the option key at all."""
    g = golden("subgc_greedy")
    ims = batch_images(g)
    res = []
    for over in (dict(), dict(decode_b16_batched=0)):
        _, _, m = _golden_model(golden, **over)
        assert m.decode_b16_batched == 0 and not m.decode_b16_on()
        del states[:]
        a = m.sample_images(_on_device(ims), opt=dict(sample_max=1, beam_size=1, return_att=1))
        b = m.sample_images(_on_device(ims), opt=dict(sample_max=1, beam_size=2))
        assert [st.S for st in states] == [40, 80] and all(st.regime == "fp32" and st.w16 is None for st in states)
        res.append((a, b))
    for x, y in zip(res[0][0] + res[0][1], res[1][0] + res[1][1]):
        for p, q in zip(x, y):
            assert torch.equal(p.view(torch.int32) if p.dtype == torch.float32 else p, q.view(torch.int32) if q.dtype == torch.float32 else q)
