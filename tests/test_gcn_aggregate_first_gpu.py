"""ops.GCN_AGGREGATE_FIRST: collection units without BatchNorm whose targets are fewer than their sources (nodes <- relations) apply
the 0/1 map to the source rows first and run fc_lft / fc_rgt on the target rows (functions.GcnAggFirstFn, include/subgc_gcn_agg_hip.h).

The reference is graph_conv_unit.py:28-36 + graph_conv.py:24-26 + the residual, restated here in fp64 (torch autograd on the CPU):
relu( A fc_rgt(fc_lft(source)) / (rowsum(A) + 1e-7) ) per role, the two roles averaged, the skip added.

The bound on the new order is not a number chosen here: on the same inputs the EXISTING order (functions.UnitPairFn + functions.GcnNodesFn)
has some maximum error against the fp64 result, and the new order must stay within 4x of it per array -- (A x) W^T against A (x W^T) is a
reassociation with the same number of roundings per element, which can move the error either way.

The bounds of the kernel-level checks (row-scaled bias epilogue, row-weighted column sums) are the a-priori bound of an fp32 sum of n
products in ANY order, |err| <= (n + 2) u sum|a_i b_i| with u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, 3.1)."""
import argparse
import functools

import pytest
import torch

from subgc import ops, synthetic
import subgc.functions as F_
import subgc.models as models
from test_packed_gpu import DEV, OPT

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
N_NODES, N_RELS = 3 + 1, 7 + 1
# (subject, object) per relation; node 3 / relation 7 are the padded dummies (gcn_backbone.py:55-67 pads with the last index).
# image 0: node 0 has MANY relations (subject of six), relation 3 has node 0 as subject AND object, node 2 is never a subject (cnt = 0)
# image 1: node 0 is never a subject, relations 2 and 5 are self loops, node 1 is the subject of four
REL = [[(0, 1), (0, 2), (0, 1), (0, 0), (0, 2), (1, 0), (0, 1), (3, 3)],
       [(1, 2), (2, 1), (1, 1), (2, 0), (1, 0), (2, 2), (1, 2), (3, 3)]]
NAMES = ("out", "dx", "dWl0", "dbl0", "dWl1", "dbl1", "dWr0", "dbr0", "dWr1", "dbr1")


@functools.lru_cache(maxsize=None)
def _case(L, Lr, B):
    """Inputs (fp32 values, kept on the CPU) and the fp64 reference results of one shape; computed once, never written to."""
    g = torch.Generator().manual_seed(1000 + L + B)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).float()
    N, K = N_NODES, N_RELS
    c = dict(L=L, Lr=Lr, B=B, N=N, K=K, rel=torch.tensor(REL[:B], dtype=torch.int64), x=rn(B, K, L), skip=rn(B, N, L), dout=rn(B, N, L))
    for r in (0, 1):
        c[f"Wl{r}"], c[f"bl{r}"] = rn(Lr, L, scale=L ** -0.5), rn(Lr, scale=0.5)
        c[f"Wr{r}"], c[f"br{r}"] = rn(L, Lr, scale=Lr ** -0.5), rn(L, scale=0.5)
    # graph_conv_unit.py:28-36 / graph_conv.py:24-26 in fp64
    d = {k: v.double().requires_grad_() for k, v in c.items() if torch.is_tensor(v) and v.is_floating_point() and k not in ("skip", "dout")}
    out = 0
    for r in (0, 1):
        F = (d["x"] @ d[f"Wl{r}"].T + d[f"bl{r}"]) @ d[f"Wr{r}"].T + d[f"br{r}"]                       # fc_rgt(fc_lft(source)) [B, K, L]
        A = torch.zeros(B, N, K, dtype=torch.float64)
        for b in range(B):
            for k in range(K):
                A[b, REL[b][k][r], k] = 1.0
        out = out + torch.relu(torch.bmm(A, F) / (A.sum(2, keepdim=True) + 1e-7))
    out = out / 2 + c["skip"].double()
    out.backward(c["dout"].double())
    ref = {"out": out.detach(), "dx": d["x"].grad}
    for r in (0, 1):
        ref.update({f"dWl{r}": d[f"Wl{r}"].grad, f"dbl{r}": d[f"bl{r}"].grad, f"dWr{r}": d[f"Wr{r}"].grad, f"dbr{r}": d[f"br{r}"].grad})
    c["ref"] = ref
    return c


def _gpu_run(c, new):
    """Output and gradients of the pair on the GPU: the aggregation-first Function, or the existing order (paired units + gcn_nodes)."""
    B, N, K, L = c["B"], c["N"], c["K"], c["L"]
    t = {k: v.to(DEV).requires_grad_(k not in ("skip", "dout")) for k, v in c.items() if torch.is_tensor(v) and v.is_floating_point()}
    rel = c["rel"].to(DEV)
    ptr, edges = ops.csr_build(rel, N)
    pw = [t[f"{w}{r}"] for w2 in ("l", "r") for r in (0, 1) for w in (f"W{w2}", f"b{w2}")]            # Wl0 bl0 Wl1 bl1 Wr0 br0 Wr1 br1
    if new:
        out = F_.GcnAggFirstFn.apply(t["x"].view(B * K, L), t["skip"], rel, ptr, edges, B, N, K, *pw)
    else:
        cat = (torch.cat([t["Wl0"], t["Wl1"]]).detach(), torch.cat([t["bl0"], t["bl1"]]).detach(), None, None, None)
        ya, yb = F_.UnitPairFn.apply(t["x"].view(B * K, L), None, cat, *pw, None, False)
        out = F_.GcnNodesFn.apply(ya.view(B, K, L), yb.view(B, K, L), t["skip"], rel, ptr, edges, N)
    out.backward(t["dout"])
    torch.cuda.synchronize()
    res = {"out": out.detach(), "dx": t["x"].grad}
    for r in (0, 1):
        res.update({f"dWl{r}": t[f"Wl{r}"].grad, f"dbl{r}": t[f"bl{r}"].grad, f"dWr{r}": t[f"Wr{r}"].grad, f"dbr{r}": t[f"br{r}"].grad})
    return {k: v.double().cpu() for k, v in res.items()}


@pytest.mark.parametrize("L,Lr,B", [(64, 32, 2), (1024, 512, 1)])
def test_new_order_is_within_4x_of_the_existing_orders_error(L, Lr, B):
    """Forward, d(source), both weight gradients and both bias gradients of both roles against the fp64 restatement.  Measured on MI355X
    (max |error| existing order / new order): see DESIGN 3, "Aggregate first"."""
    c = _case(L, Lr, B)
    old, new = _gpu_run(c, False), _gpu_run(c, True)
    errs = {}
    for k in NAMES:
        ref = c["ref"][k].reshape(old[k].shape)
        errs[k] = (float((old[k] - ref).abs().max()), float((new[k] - ref).abs().max()), float(ref.abs().max()))
        print(f"L={L} {k:5s} max|ref| {errs[k][2]:.3e}  existing order {errs[k][0]:.3e}  aggregate first {errs[k][1]:.3e}")
    for k, (e_old, e_new, top) in errs.items():
        assert top > 0 and e_new <= 4.0 * e_old, (k, e_old, e_new)


def test_a_row_without_neighbours_is_exactly_zero_bias_included():
    """cnt = 0 (image 0, node 2 as subject; image 1, node 0): aggregated row, bias scale, H and Y of that role are exact zeros, its ReLU
    mask lets nothing through, and a bias gradient ignores whatever stands in that row."""
    c = _case(64, 32, 2)
    B, N, K, L = c["B"], c["N"], c["K"], c["L"]
    rel = c["rel"].to(DEV)
    ptr, edges = ops.csr_build(rel, N)
    x = c["x"].to(DEV)
    A0, A1, s0, s1 = ops.gcn_agg_fwd(x.view(B * K, L), ptr, edges, B, N, K, L)
    rows = [0 * N + 2, 1 * N + 0]
    cnt0 = torch.tensor([[sum(1 for k in range(K) if REL[b][k][0] == n) for n in range(N)] for b in range(B)], dtype=torch.float32).flatten()
    assert all(float(cnt0[r]) == 0.0 for r in rows) and float(cnt0.max()) == 6.0
    assert torch.equal(s0.cpu(), 0.5 * cnt0 / (cnt0 + torch.tensor(1e-7, dtype=torch.float32)))
    H0, H1 = (torch.empty(B * N, c["Lr"], device=DEV) for _ in range(2))
    ops.gemm_pair_rowbias(A0, A1, c["Wl0"].to(DEV), c["Wl1"].to(DEV), H0, H1, tb=True, bias1=c["bl0"].to(DEV), bias2=c["bl1"].to(DEV), scale1=s0, scale2=s1)
    Y0, Y1 = (torch.empty(B * N, L, device=DEV) for _ in range(2))
    ops.gemm_pair_rowbias(H0, H1, c["Wr0"].to(DEV), c["Wr1"].to(DEV), Y0, Y1, tb=True, bias1=c["br0"].to(DEV), bias2=c["br1"].to(DEV), scale1=s0, scale2=s1,
                          relu=True)
    dout = c["dout"].to(DEV).view(B * N, L)
    dY0, dY1 = ops.gcn_agg_relu_bwd(dout, Y0, Y1)
    for r in rows:
        for name, a in (("Xagg", A0), ("H", H0), ("Y", Y0), ("dY", dY0)):
            assert not bool(a[r].any()), (name, r)
        assert float(s0[r]) == 0.0 and bool(Y1[r].any())                   # the other role of the same node is alive
    big = dout.clone()
    big[rows] = 1e30
    db, db_big = torch.empty(L, device=DEV), torch.empty(L, device=DEV)
    ops.colsum_rows((dout,), (s0,), (db,))
    ops.colsum_rows((big,), (s0,), (db_big,))
    assert torch.equal(db, db_big) and bool(db.any())


def test_backward_gather_accumulates_into_what_holds_the_source_gradient():
    c = _case(64, 32, 2)
    B, N, K, L = c["B"], c["N"], c["K"], c["L"]
    rel = c["rel"].to(DEV)
    ptr, _ = ops.csr_build(rel, N)
    g = torch.Generator().manual_seed(5)
    dA0, dA1 = (torch.randn(B * N, L, generator=g).to(DEV) for _ in range(2))
    base = torch.randn(B * K, L, generator=g).to(DEV)
    fresh = ops.gcn_agg_bwd(dA0, dA1, rel, ptr, B, N, K, L)
    acc = ops.gcn_agg_bwd(dA0, dA1, rel, ptr, B, N, K, L, out=base.clone())
    cnt = torch.tensor([[[sum(1 for k in range(K) if REL[b][k][r] == n) for n in range(N)] for b in range(B)] for r in (0, 1)], dtype=torch.float64)
    w = 0.5 / (cnt + 1e-7)
    ref = torch.zeros(B, K, L, dtype=torch.float64)
    for b in range(B):
        for k in range(K):
            s, o = REL[b][k]
            ref[b, k] = w[0, b, s] * dA0.double().cpu()[b * N + s] + w[1, b, o] * dA1.double().cpu()[b * N + o]
    bound = 4 * U * (w.max() * (dA0.abs().max() + dA1.abs().max())).item()     # two products, one sum, the fp32 weight: a few roundings
    assert float((fresh.double().cpu().view(B, K, L) - ref).abs().max()) <= bound
    assert float((acc.double().cpu().view(B, K, L) - ref - base.double().cpu().view(B, K, L)).abs().max()) <= bound + 2 * U * float(ref.abs().max() + base.abs().max())


@pytest.mark.parametrize("M,N,K,relu", [(70, 64, 96, False), (70, 64, 96, True), (64, 64, 2048, False), (256, 256, 2048, False), (300, 100, 50, False)])
def test_row_scaled_bias_epilogue(M, N, K, relu):
    """C = [relu](A W^T + s[row] bias) against fp64: M = 70 is a ragged last tile, K = 2048 the split-K shapes (256 x 256 takes eight K
    parts and the reduce pass), N = 100 the scalar epilogue; a NULL scale is the existing entry point bit for bit."""
    g = torch.Generator().manual_seed(M + N + K)
    A, W, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    s = torch.rand(M, generator=g)
    s[::7] = 0.0
    ref = A.double() @ W.double().T + s.double()[:, None] * bias.double()
    mag = A.double().abs() @ W.double().abs().T + (s.double()[:, None] * bias.double()).abs()
    if relu:
        ref = torch.relu(ref)
    Ad, Wd, bd, sd = (t.to(DEV) for t in (A, W, bias, s))
    C = torch.empty(M, N, device=DEV)
    ops.gemm_rowbias(Ad, Wd, C, tb=True, bias=bd, bias_scale=sd, relu=relu)
    err = (C.double().cpu() - ref).abs()
    print(f"M={M} N={N} K={K}: max error {float(err.max()):.3e}, bound at that element {float(((K + 2) * U * mag).flatten()[err.argmax()]):.3e}")
    assert bool((err <= (K + 2) * U * mag).all())
    # pair form: the same two products in one launch, scales swapped between the problems
    s2 = sd.flip(0).contiguous()
    C1, C2, D2 = (torch.empty(M, N, device=DEV) for _ in range(3))
    ops.gemm_pair_rowbias(Ad, Ad, Wd, Wd, C1, C2, tb=True, bias1=bd, bias2=bd, scale1=sd, scale2=s2, relu=relu)
    ops.gemm_rowbias(Ad, Wd, D2, tb=True, bias=bd, bias_scale=s2, relu=relu)
    ref2 = A.double() @ W.double().T + s.flip(0).double()[:, None] * bias.double()
    ref2 = torch.relu(ref2) if relu else ref2
    assert bool(((C1.double().cpu() - ref).abs() <= (K + 2) * U * mag).all())
    assert bool(((C2.double().cpu() - ref2).abs() <= (K + 2) * U * (mag + bias.double().abs())).all())
    # NULL scale: subgc_gemm_f32 / subgc_gemm_f32_pair themselves (their tiled forms: the weight-streaming form for M <= 80 is a different kernel)
    E1, E2, P1, P2, Q1, Q2 = (torch.empty(M, N, device=DEV) for _ in range(6))
    with ops.gemm_tune(no_skinny=True):
        ops.gemm(Ad, Wd, E1, tb=True, bias=bd, relu=relu)
        ops.gemm_rowbias(Ad, Wd, E2, tb=True, bias=bd, relu=relu)
        assert torch.equal(E1, E2)
        if not relu:
            ops.gemm_pair(Ad, Ad, Wd, Wd, P1, P2, tb=True, bias1=bd, bias2=bd)
            ops.gemm_pair_rowbias(Ad, Ad, Wd, Wd, Q1, Q2, tb=True, bias1=bd, bias2=bd)
            assert torch.equal(P1, Q1) and torch.equal(P2, Q2)


@pytest.mark.parametrize("M,N", [(70, 64), (300, 1024), (64, 100)])
def test_row_weighted_column_sums(M, N):
    g = torch.Generator().manual_seed(M * N)
    X0, X1, w0, w1 = torch.randn(M, N, generator=g), torch.randn(M, N, generator=g), torch.rand(M, generator=g), torch.rand(M, generator=g)
    w0[::5] = 0.0
    base = torch.randn(2, N, generator=g)
    refs = [(w.double()[:, None] * X.double()).sum(0) for X, w in ((X0, w0), (X1, w1))]
    mags = [(w.double()[:, None] * X.double()).abs().sum(0) for X, w in ((X0, w0), (X1, w1))]
    d = [t.to(DEV) for t in (X0, X1, w0, w1)]
    o = [torch.empty(N, device=DEV) for _ in range(2)]
    ops.colsum_rows(d[:2], d[2:], o)
    acc = [b.to(DEV).clone() for b in base]
    ops.colsum_rows(d[:2], d[2:], acc, accumulate=True)
    one = torch.empty(N, device=DEV)
    ops.colsum_rows(d[1:2], d[3:4], (one,))
    again = [torch.empty(N, device=DEV) for _ in range(2)]
    ops.colsum_rows(d[:2], d[2:], again)
    for q in (0, 1):
        assert bool(((o[q].double().cpu() - refs[q]).abs() <= (M + 2) * U * mags[q]).all())
        assert bool(((acc[q].double().cpu() - refs[q] - base[q].double()).abs() <= (M + 3) * U * (mags[q] + base[q].double().abs())).all())
        assert torch.equal(o[q], again[q])                                  # a fixed order: the same bits every time
    assert torch.equal(one, o[1])


@functools.lru_cache(maxsize=None)
def _model_runs():
    """One small Sub-GC model (no BatchNorm, 37 node rows against 65 relation rows per image), one train step in deterministic mode under:
    the switch on, the switch off, and the dispatch of the parent (the aggregation-first choice removed altogether)."""
    torch.manual_seed(0)
    m = models.setup(argparse.Namespace(**OPT)).to(DEV).train()
    batch = {k: v.to(DEV) for k, v in synthetic.make_train_batch(4, D=256, vocab=300, n_obj_cls=60, seed=9, fc_size=256, min_len=2, max_len=16).items()}
    real_ok, real_call = F_.gcn_aggregate_first_ok, ops.call_gcn_agg
    res = {}
    for mode in ("on", "off", "parent"):
        calls = []

        def spy(name, *a):
            calls.append(name)
            return real_call(name, *a)

        ops.GCN_AGGREGATE_FIRST = mode == "on"
        ops.call_gcn_agg = spy
        if mode == "parent":
            F_.gcn_aggregate_first_ok = lambda *a: False
        try:
            with ops.deterministic():
                m.packed_decoder = True
                lw = models.LossWrapper(m, None)
                m.flatten_grads()
                b = batch
                out = lw(b["fc_feats"], b["att_feats"], b["labels"], b["masks"], b["att_masks"], None, None, None, b["obj_dist"], None, b["rel_ind"],
                         None, b["pred_dist"], b["gpn_obj_ind"], b["gpn_pred_ind"], b["gpn_nrel_ind"], b["gpn_pool_mtx"])
                models.total_loss(out).backward()
                torch.cuda.synchronize()
        finally:
            ops.GCN_AGGREGATE_FIRST, ops.call_gcn_agg, F_.gcn_aggregate_first_ok = True, real_call, real_ok
        res[mode] = (float(out["lang_loss"].detach()), m.flat_grads.clone(), calls)
    return res


def test_switch_off_is_the_parents_path_bit_for_bit():
    res = _model_runs()
    (l_off, g_off, c_off), (l_par, g_par, c_par) = res["off"], res["parent"]
    assert c_off == [] and c_par == []                                       # none of the new entry points is reached
    assert l_off == l_par and torch.equal(g_off, g_par)


def test_switch_on_takes_the_new_order_and_agrees_with_the_old():
    """The train step with the switch on against the switch off: the project's own bound for a reordered fp32 sum (tests/test_packed_gpu.py:47-49,
    as tests/test_zero_state_gpu.py uses it)."""
    res = _model_runs()
    (l_on, g_on, c_on), (l_off, g_off, _) = res["on"], res["off"]
    assert c_on.count("subgc_gcn_agg_fwd") == 1 and c_on.count("subgc_gcn_agg_bwd") == 1 and c_on.count("subgc_gemm_f32_pair_rowbias") == 2
    assert c_on.count("subgc_colsum_rows_f32") == 2 and c_on.count("subgc_gcn_agg_relu_bwd") == 1
    top = float(g_off.abs().max())
    print(f"loss off {l_off!r} on {l_on!r}  max |dg| {float((g_on - g_off).abs().max()):.3e}  max |g| {top:.3e}")
    assert abs(l_on - l_off) <= 2e-5 * max(1.0, abs(l_off))
    torch.testing.assert_close(g_on, g_off, atol=2e-5 * top + 1e-7, rtol=2e-4)
