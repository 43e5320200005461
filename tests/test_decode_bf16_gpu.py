"""The bf16 decode step (compute_dtype = bf16) in each of its three row regimes (functions.DecodeState):

  <= 16 rows   both LSTM matrices, h2att and the logit layer streamed as bf16 twins (subgc_lstm_step_skinny MT = 1, subgc_gemm_skinny_wb16);
  17 .. 32     only the LSTM matrices in bf16 (subgc_lstm_step_skinny MT = 2), h2att and logits on the fp32 GEMM;
  > 32         fp32 throughout (unfused step).

Kernels are compared with an fp64 product over the bf16-ROUNDED weights and the fp32 activations, so the only error left is fp32
accumulation order and the fp32 tolerances of the other skinny tests apply.  One decode step per regime is compared with the oracle's
core step fed fp64 parameters in which exactly the matrices that regime streams are the model's own bf16 twins: a wrong twin, a
swapped half or a regime that streams the other precision moves the log-probs by 2e-4 .. 8e-3, past those tolerances.  The model-level
paths (graphed / eager, fused / separate pick, top-k, forced, tap, beam, multi-image batches) are compared with the fp32 oracle along
the same token path at the bf16 tolerance, and every greedy path with the fused-pick anchor at fp32 rounding."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import subgc_oracle as O
from subgc import functions as F_
from subgc import ops, synthetic
from test_parity_gpu import DEV, build, close

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------ kernels against fp64
@pytest.mark.parametrize("N", [16, 1000, 1003, 9488])
@pytest.mark.parametrize("K", [4, 52, 1000, 2048])
def test_gemm_skinny_wb16_equals_fp64_on_rounded_weights(N, K):
    """subgc_gemm_skinny_wb16: N % 16 != 0 leaves a partial last workgroup, K % 8 == 4 gives bf16 rows that are only 8-byte aligned;
    contiguous and strided A (lda > K), a W view with ldw = K + 4, with and without bias and ReLU; rows past M and columns past N of
    the output stay untouched."""
    g = torch.Generator().manual_seed(N * 7 + K)
    Wbuf = (torch.randn(N, K + 4, generator=g) * K ** -0.5).to(DEV).to(BF)
    Wv = Wbuf[:, :K]                                                                # ldw = K + 4
    Wc = Wv.contiguous()
    bias = torch.randn(N, generator=g).to(DEV)
    Abuf = torch.randn(16, K + 8, generator=g).to(DEV)
    for M in (1, 7, 16):
        for strided, with_bias, relu in ((False, False, False), (True, True, False), (True, True, True), (False, False, True), (False, True, False)):
            A = Abuf[:M, :K] if strided else Abuf[:M, :K].contiguous()
            W = Wv if strided else Wc
            out = torch.full((M + 2, N + 5), 7.0, device=DEV)
            ops.gemm_skinny_wb16(A, W, out[:M, :N], bias=bias if with_bias else None, relu=relu)
            ref = A.double() @ W.double().t()
            if with_bias:
                ref = ref + bias.double()
            if relu:
                ref = ref.clamp_min(0)
            torch.testing.assert_close(out[:M, :N].double(), ref, atol=3e-5, rtol=1e-5, msg=lambda s: f"M={M} {strided} {with_bias} {relu}: {s}")
            assert float(out[M:].min()) == 7.0 and float(out[M:].max()) == 7.0                      # sentinel rows
            assert float(out[:, N:].min()) == 7.0 and float(out[:, N:].max()) == 7.0                # sentinel columns


def _lstm_ref(x, W, b0, b1, add1_rows, add2, cp):
    pre = x.double() @ W.double().t()
    for t in (b0, b1, add1_rows, add2):
        if t is not None:
            pre = pre + t.double()
    R = W.size(0) // 4
    i, f, gg, o = pre[:, :R].sigmoid(), pre[:, R:2 * R].sigmoid(), pre[:, 2 * R:3 * R].tanh(), pre[:, 3 * R:].sigmoid()
    cn = i * gg + (f * cp.double() if cp is not None else 0.0)
    return cn, o * cn.tanh()


@pytest.mark.parametrize("R", [48, 52, 1000])
@pytest.mark.parametrize("kmul", [1, 2, 3])
def test_fused_lstm_step_with_bf16_weights_equals_fp64(R, kmul):
    """subgc_lstm_step_skinny with bf16 w_perm (the fused decode step's bf16 snapshot), S = 1 .. 16 (MT = 1) and 17 .. 32 (MT = 2):
    test_fused_lstm_step_equals_gemm_plus_cell with bf16 weights -- the x -> gates table path (tokens -1 and past the table clamp) and the
    add1 path, add2, three h destinations inside wider buffers, c_prev = None -- plus w_perm as a column slice of a padded snapshot
    (functions._cat_weights: ldw > K) and S = 0."""
    K = kmul * R
    g = torch.Generator().manual_seed(R * 10 + kmul)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(DEV)
    W = rnd(4 * R, K, sc=K ** -0.5).to(BF)                                         # the reference reads the ROUNDED weights
    perm = ops.lstm_gate_perm(R, DEV)
    Wp = W[perm].contiguous()
    snap = ops.act_padded((4 * R, (R + K + 7) // 8 * 8), DEV, True)                 # [R columns | w_perm | pad to the pitch], like Wc2[:, R:]
    ops.copy2d(W[perm], snap[:, R:R + K])
    Wslice = snap[:, R:R + K]
    assert ops.ld(Wslice) > K
    b0, b1 = rnd(4 * R, sc=0.3), rnd(4 * R, sc=0.3)
    table = rnd(23, 4 * R, sc=0.5)
    for S in (1, 10, 16, 17, 24, 32):
        x, add2, cp = rnd(S, K), rnd(S, 4 * R, sc=0.5), rnd(S, R)
        tok = torch.randint(-1, 25, (S,), generator=g).to(DEV)
        rows = table[tok.clamp(0, 22)]
        for use_tok, w in ((True, Wp), (False, Wp), (True, Wslice)):
            c = torch.full((S, R), 5.0, device=DEV)
            wide = torch.full((S, 3 * R), 9.0, device=DEV)
            wide2 = torch.full((S, 2 * R + 4), 9.0, device=DEV)
            wide3 = torch.full((S + 1, R + 8), 9.0, device=DEV)
            hs = [wide[:, R:2 * R], wide2[:, R + 4:], wide3[:S, 4:R + 4]]
            add1 = table if use_tok else rows.contiguous()
            ops.lstm_step_skinny(x, w, cp, c, hs, b0, b1, add1, tok if use_tok else None, add2)
            cn, hn = _lstm_ref(x, W, b0, b1, rows, add2, cp)
            torch.testing.assert_close(c.double(), cn, atol=2e-5, rtol=1e-5)
            torch.testing.assert_close(hs[0].double(), hn, atol=2e-5, rtol=1e-5)
            assert torch.equal(hs[1], hs[0]) and torch.equal(hs[2], hs[0])
            assert float(wide[:, :R].min()) == 9.0 and float(wide[:, 2 * R:].max()) == 9.0 and float(wide[:, 2 * R:].min()) == 9.0
            assert float(wide2[:, :R + 4].min()) == 9.0 and float(wide2[:, :R + 4].max()) == 9.0
            assert float(wide3[S].min()) == 9.0 and float(wide3[:, :4].max()) == 9.0 and float(wide3[:, R + 4:].min()) == 9.0
        c2, h2 = torch.empty(S, R, device=DEV), torch.empty(S, R, device=DEV)       # no additive terms, no c_prev
        ops.lstm_step_skinny(x, Wp, None, c2, [h2])
        cn, hn = _lstm_ref(x, W, None, None, None, None, None)
        torch.testing.assert_close(c2.double(), cn, atol=2e-5, rtol=1e-5)
        torch.testing.assert_close(h2.double(), hn, atol=2e-5, rtol=1e-5)
    # S = 0: nothing is written
    c, h = torch.full((4, R), 3.0, device=DEV), torch.full((4, R), 3.0, device=DEV)
    ops.lstm_step_skinny(rnd(4, K)[:0], Wp, rnd(4, R), c[:0], [h[:0]], b0, b1, table, tok[:0], rnd(4, 4 * R)[:0])
    torch.cuda.synchronize()
    assert float(c.min()) == 3.0 and float(c.max()) == 3.0 and float(h.min()) == 3.0 and float(h.max()) == 3.0


# ------------------------------------------------------------------------------------------------ one step per regime vs the oracle
def _twin(m, name):
    return m.W16(name, m.weights_b16()).double().cpu()


def _oracle_params(m, w, S):
    """fp64 parameters with the matrices the S-row regime streams replaced by the model's bf16 twins."""
    P = {k: torch.from_numpy(v).double() for k, v in w.items()}
    R = m.rnn_size
    if S <= 32:
        P["core.att_lstm.weight_ih"][:, :R] = _twin(m, "core.att_lstm.weight_ih")[:, :R]
        for k in ("core.att_lstm.weight_hh", "core.lang_lstm.weight_ih", "core.lang_lstm.weight_hh"):
            P[k] = _twin(m, k)
    if S <= 16:
        for k in ("core.attention.h2att.weight", "logit.weight"):
            P[k] = _twin(m, k)
    return P


@pytest.mark.parametrize("S", [1, 16, 17, 32, 33])
def test_one_bf16_decode_step_per_regime_equals_the_oracle_on_rounded_weights(golden, S):
    g = golden("subgc_greedy")
    w = golden("subgc_train").group("weights")
    m = build(g, w, False, compute_dtype="bf16")
    R, V1 = m.rnn_size, m.vocab_size + 1
    gen = torch.Generator().manual_seed(40 + S)
    Nn = 7
    fc = torch.randn(S, m.P("fc_embed.0.weight").size(1), generator=gen)
    att = torch.randn(S, Nn, m.P("att_embed.0.weight").size(1), generator=gen)
    lens = torch.randint(1, Nn + 1, (S,), generator=gen)
    lens[0] = Nn
    masks = (torch.arange(Nn).view(1, Nn) < lens.view(-1, 1)).float()
    p_fc, p_att, pp_att, p_masks = m._prepare_feature(fc.to(DEV), att.to(DEV), masks.to(DEV))   # stepapi.prepare_feature
    n_max = p_att.size(1)
    pr = SimpleNamespace(S=S, N=n_max, f=p_fc.contiguous(), u=pp_att.contiguous().view(S * n_max, -1), v=p_att.contiguous().view(S * n_max, R),
                         off=(torch.arange(S, device=DEV, dtype=torch.int32) * n_max).contiguous(), lens=p_masks.sum(1).to(torch.int32).contiguous())
    st = F_.DecodeState(pr, m._decoder_params(), n_max, True, xt_table=m.xt_gates_table(), fuse_lstm=True, W16=m.decode_w16())
    if S <= 16:
        assert st.w16 is not None and st.Wc1.dtype == BF and st.Wc2.dtype == BF and st.lg_op.dtype == BF
    elif S <= 32:
        assert st.w16 is not None and st.Wc1.dtype == BF and st.Wc2.dtype == BF and st.lg_op.dtype == torch.float32
    else:
        assert not st.fused and st.w16 is None and st.Wc1.dtype == torch.float32 and st.lg_op.dtype == torch.float32
    h = torch.randn(2, S, R, generator=gen) * 0.3
    c = torch.randn(2, S, R, generator=gen) * 0.3
    hd, cd = h.to(DEV), c.to(DEV)
    st.H1[:, :R] = hd[1]; st.H1[:, R:] = hd[0]                                      # stepapi.get_logprobs_state's state layout
    st.H2[:, 2 * R:] = hd[1]
    st.C1[0].copy_(cd[0]); st.C2[0].copy_(cd[1])
    toks = torch.randint(0, V1, (3, S), generator=gen)
    cfg = O.Cfg(g.opt())
    f, v, u, mk = p_fc.double().cpu(), p_att.double().cpu(), pp_att.double().cpu(), p_masks.cpu()

    def oracle(P):
        state, out = ((h[0].double(), h[1].double()), (c[0].double(), c[1].double())), []
        for t in range(3):
            lp, state, a = O.core_step(P, cfg, toks[t], f, v, u, mk, state, False)
            out.append((lp, state, a))
        return out

    P = _oracle_params(m, w, S)
    want = oracle(P)
    alpha = torch.zeros(S, n_max, device=DEV)
    for t in range(3):
        lp = st.step(toks[t].to(DEV), alpha, normalize=True)
        wlp, ((h1, h2), (c1, c2)), wa = want[t]
        close(lp, wlp, f"logprobs step {t}", atol=1e-4, rtol=1e-5)
        close(st.H1[:, R:], h1, f"h_att step {t}", atol=1e-4, rtol=1e-5)
        close(st.H1[:, :R], h2, f"h_lang step {t}", atol=1e-4, rtol=1e-5)
        close(st.C1[0], c1, f"c_att step {t}", atol=1e-4, rtol=1e-5)
        close(st.C2[0], c2, f"c_lang step {t}", atol=1e-4, rtol=1e-5)
        close(alpha, wa, f"alpha step {t}", atol=1e-5, rtol=1e-5)
    # the comparison can tell the precisions apart: streaming the other precision of any one of these matrices moves the log-probs past the
    # 1e-4 tolerance (measured: 2e-4 for h2att at S = 1, 1e-3 .. 8e-3 otherwise)
    full = {k: torch.from_numpy(v_).double() for k, v_ in w.items()}
    for k in ("logit.weight", "core.attention.h2att.weight", "core.lang_lstm.weight_ih", "core.att_lstm.weight_hh"):
        other = dict(P, **{k: _twin(m, k) if torch.equal(P[k], full[k]) else full[k]})
        assert float((oracle(other)[2][0] - want[2][0]).abs().max()) > 1.5e-4, k


# ------------------------------------------------------------------------------------------------ model-level decode paths in bf16
@pytest.fixture
def states(monkeypatch):
    """Every DecodeState built while the test runs (the graphed loops build theirs at capture)."""
    seen = []
    orig = F_.DecodeState.__init__

    def rec(self, *a, **kw):
        orig(self, *a, **kw)
        seen.append(self)

    monkeypatch.setattr(F_.DecodeState, "__init__", rec)
    return seen


def _regime(st):
    if st.w16 is None:
        return "fp32"
    assert st.Wc1.dtype == BF and st.Wc2.dtype == BF
    return "bf16" if st.lg_op.dtype == BF else "lstm-bf16"


def _upto_eos(seq):
    """[n, T] bool: the steps whose token was picked while the row was unfinished (its <eos> included)."""
    alive = torch.ones_like(seq, dtype=torch.bool)
    alive[:, 1:] = (seq[:, :-1] > 0).cumprod(1).bool()
    return alive


def _same_path_as_oracle(ret, orc, tb, sopt, min_same):
    """The fp32 oracle teacher-forced with the product's tokens: log-probs within 5e-2 (bf16), attention within 2e-2 and its arg-max equal
    where the oracle's top-1 / top-2 margin exceeds 4e-2; where the free-running oracle takes another word, its margin over the product's
    word at the first differing step is below 0.1 (= tokens equal wherever that margin exceeds 0.1)."""
    seq = ret[0].cpu()
    forced = orc.sample(*synthetic.sample_args(tb), opt=sopt, forced=seq)
    free = orc.sample(*synthetic.sample_args(tb), opt=sopt)
    np.testing.assert_array_equal(ret[3].cpu().numpy(), forced[3].numpy())
    live = _upto_eos(seq)
    close(ret[1].cpu()[live], forced[1][live], "seqLogprobs vs oracle", atol=5e-2, rtol=0)
    if len(ret) > 4:
        assert tuple(ret[4].shape) == tuple(forced[4].shape)
        close(ret[4], forced[4], "att2_weights vs oracle", atol=2e-2, rtol=0)
        top2 = forced[4].topk(2, -1).values
        sure = (top2[..., 0] - top2[..., 1]) > 4e-2
        assert int(sure.sum()) > 10 and bool((ret[4].cpu().argmax(-1)[sure] == forced[4].argmax(-1)[sure]).all())
    same = 0
    for r in range(seq.size(0)):
        diff = (free[0][r] != seq[r]).nonzero()
        if diff.numel() == 0:
            same += 1
            continue
        t0 = int(diff[0])
        assert float(free[1][r, t0] - forced[1][r, t0]) < 0.1, (r, t0)
    assert same >= min_same


def _greedy_case(golden, **over):
    g = golden("subgc_greedy")
    w = golden("subgc_train").group("weights")
    tb = g.tensors("inputs")
    return g, w, tb, lambda: build(g, w, False, compute_dtype="bf16", **over)


def _run(m, tb, sopt, **kw):
    return m(*synthetic.sample_args({k: v.to(DEV) for k, v in tb.items()}), opt=sopt, mode="sample", **kw)


@pytest.mark.parametrize("return_att", [0, 1])
def test_bf16_greedy_paths_equal_the_fused_pick_anchor_and_the_oracle(golden, states, return_att):
    """Greedy decode of one image (10 sub-graphs: the <= 16-row regime) through every path: the graphed fused pick (anchor), the separate
    pick, the eager loop, a forced decode and a decode with m.tap set.  Each against the fp32 oracle along its own token path, and each
    equal to the anchor: tokens and kept sub-graphs identical, log-probs within 2e-5."""
    g, w, tb, mk = _greedy_case(golden)
    sopt = dict(sample_max=1, beam_size=1, return_att=return_att)
    orc = O.Oracle(g.opt(), w)
    m = mk()
    anchor = _run(m, tb, sopt)
    loops = [x for x in m._graph_cache.values() if hasattr(x, "st")]
    assert loops and all(_regime(x.st) == "bf16" for x in loops)
    _same_path_as_oracle(anchor, orc, tb, sopt, min_same=5)
    n = anchor[0].size(0)
    assert n <= 16
    live = _upto_eos(anchor[0].cpu())
    results = {}
    m = mk(); m.decode_fused_pick = False
    results["separate pick"] = _run(m, tb, sopt)
    m = mk(); m.decode_hipgraph = False
    results["eager"] = _run(m, tb, sopt)
    m = mk()
    results["forced"] = _run(m, tb, sopt, forced=anchor[0])
    m = mk(); m.tap = {}
    results["tap"] = _run(m, tb, sopt)
    # the tap run saw every step's log-probs: the picks of this seed have top-2 margins far above the fp32 rounding of two kernels
    lp = m.tap["step_logp"][:anchor[0].size(1)].permute(1, 0, 2).cpu()
    top2 = lp.topk(2, -1).values
    margin = (top2[..., 0] - top2[..., 1])[live]
    assert float(margin.min()) > 1e-4, float(margin.min())
    assert states and all(_regime(st) == "bf16" for st in states)
    for name, r in results.items():
        assert torch.equal(r[0], anchor[0]) and torch.equal(r[3], anchor[3]), name
        if name == "forced":                                                       # a forced path keeps scoring its tokens after <eos>
            close(r[1].cpu()[live], anchor[1].cpu()[live], name, atol=2e-5, rtol=1e-5)
        else:
            close(r[1], anchor[1], name, atol=2e-5, rtol=1e-5)
        close(r[2], anchor[2], name + " score", atol=1e-6, rtol=1e-6)
        if return_att:
            assert tuple(r[4].shape) == tuple(anchor[4].shape), name
            close(r[4], anchor[4], name + " att", atol=1e-6, rtol=1e-5)
        _same_path_as_oracle(r, orc, tb, sopt, min_same=5)


@pytest.mark.parametrize("graphed", [True, False])
def test_bf16_topk_sampling_with_injected_uniforms_follows_the_oracle(golden, states, graphed):
    """Top-k sampling (the step's separate pick, both on the replayed loop and eagerly) with injected uniforms against the fp32 oracle drawing
    from the same uniforms.  A sampled path may fork where bf16 rounding can move the draw: every fork is explained at its first differing
    step, where both paths share their history, from the oracle's top-k distribution there -- either the uniform sits near a cumulative-
    probability boundary and the two words are neighbours across it (test_shapes_gpu's explanation, its 1e-4 boundary tolerance widened
    to 5e-2, the bf16 log-prob tolerance), or the two words are both in the top k with tempered log-probs within 2 x 5e-2 / temp of each
    other, so that bf16 rounding can swap their order in the cumulative sum.  Along the product's own path the oracle's log-probs match
    within 5e-2."""
    g = golden("subgc_topk")
    w = golden("subgc_train").group("weights")
    tb = g.tensors("inputs")
    sopt = g.meta["sample_opt"]
    m = build(g, w, False, compute_dtype="bf16")
    if not graphed:
        m.decode_hipgraph = False
    n = g.group("out")["seq"].shape[0]
    u = torch.rand(n, m.seq_length, generator=torch.Generator().manual_seed(11))
    ret = _run(m, tb, sopt, uniforms=u.to(DEV))
    assert states and all(_regime(st) == "bf16" for st in states)
    if graphed:
        assert [x for x in m._graph_cache.values() if hasattr(x, "st")]
    orc = O.Oracle(g.opt(), w)
    tap = {}
    want = orc.sample(*synthetic.sample_args(tb), opt=sopt, uniforms=u, tap=tap)
    forced = orc.sample(*synthetic.sample_args(tb), opt=sopt, forced=ret[0].cpu())
    np.testing.assert_array_equal(ret[3].cpu().numpy(), want[3].numpy())
    got = ret[0].cpu()
    live = _upto_eos(got)
    close(ret[1].cpu()[live], forced[1][live], "topk seqLogprobs vs oracle", atol=5e-2, rtol=0)
    same = (got == want[0]).all(1)
    assert int(same.sum()) >= n // 2
    for r in (~same).nonzero().flatten().tolist():
        t0 = int((got[r] != want[0][r]).nonzero()[0])
        top, idx = tap["topk_lp"][t0][r].double(), tap["topk_idx"][t0][r].tolist()
        words = {int(got[r, t0]), int(want[0][r, t0])}
        cdf = torch.softmax(top, 0).cumsum(0)
        gaps = (cdf[:-1] - float(u[r, t0])).abs()
        j = int(gaps.argmin())
        boundary = float(gaps[j]) < 5e-2 and words <= {idx[j], idx[j + 1], 0}
        swap = words <= set(idx) and float((top[idx.index(max(words))] - top[idx.index(min(words))]).abs()) < 2 * 5e-2 / m.topk_temp
        assert boundary or swap, (r, t0, idx, top.tolist(), cdf.tolist(), float(u[r, t0]), words)


def test_bf16_sct_and_beam_decodes(golden, states):
    """sct (eager loop, <= 16 rows: the bf16 regime) against the oracle; beam 2 pins today's contract that beam search streams the fp32
    weights (functions.DecodeState without W16) and follows the oracle along its top beam's tokens."""
    g = golden("subgc_sct")
    w = golden("subgc_train").group("weights")
    tb = g.tensors("inputs")
    sopt = g.meta["sample_opt"]
    ret = _run(build(g, w, False, compute_dtype="bf16"), tb, sopt)
    assert states and all(_regime(st) == "bf16" for st in states)
    _same_path_as_oracle(ret, O.Oracle(g.opt(), w), tb, sopt, min_same=5)
    del states[:]
    g, w, tb, mk = _greedy_case(golden)
    ret = _run(mk(), tb, dict(sample_max=1, beam_size=2))
    assert states and all(_regime(st) == "fp32" for st in states)
    orc = O.Oracle(g.opt(), w)
    forced = orc.sample(*synthetic.sample_args(tb), opt=dict(sample_max=1, beam_size=1), forced=ret[0].cpu())
    np.testing.assert_array_equal(ret[3].cpu().numpy(), forced[3].numpy())
    live = _upto_eos(ret[0].cpu())
    close(ret[1].cpu()[live], forced[1][live], "beam seqLogprobs vs oracle", atol=5e-2, rtol=0)


@pytest.mark.parametrize("images,rows,regime", [((1, 4, 5), 12, "bf16"), ((0, 1, 3), 26, "lstm-bf16"), ((0, 2, 3, 6), 40, "fp32")])
def test_bf16_sample_images_batches_in_each_row_regime(golden, states, images, rows, regime):
    """Cross-image decode batches (sample_images, the eager loop) whose rows total <= 16, 17 .. 32 and > 32: each runs its regime, and each
    image's captions follow the fp32 oracle."""
    g = golden("subgc_greedy")
    w = golden("subgc_train").group("weights")
    m = build(g, w, False, compute_dtype="bf16")
    D = g.meta["opt"]["att_feat_size"]
    spec = [(24, 14), (3, None), (40, 10), (9, 12), (1, None), (2, None), (5, None)]      # test_parity_gpu's images; 10, 6, 10, 10, 2, 4, 10 rows
    ims = [synthetic.make_test_batch(spec[i][0], D=D, seed=300 + i, fc_size=D, node_pool=spec[i][1]) for i in images]
    sopt = dict(sample_max=1, beam_size=1)
    out = m.sample_images([{k: v.to(DEV) for k, v in b.items()} for b in ims], opt=sopt)
    assert sum(r[0].size(0) for r in out) == rows
    assert [st.S for st in states] == [rows] and _regime(states[0]) == regime
    orc = O.Oracle(g.opt(), w)
    for r, b in zip(out, ims):
        _same_path_as_oracle(r, orc, b, sopt, min_same=r[0].size(0) // 2)
