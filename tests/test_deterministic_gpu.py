"""Deterministic mode (subgc_deterministic / ops.deterministic) on the MI355X: every rewritten reduction repeats bit for bit under
contention, gives the same bits at any pointer alignment and workspace size, agrees with an fp64 CPU sum, and whole training runs
(dropout on, FlatAdam) repeat exactly while still matching the goldens."""
import argparse
import ctypes
import re

import numpy as np
import pytest
import torch

from subgc import _lib, ops, parallel, synthetic
import subgc.models as models
from test_parity_gpu import DEV, build, close, run_train  # noqa: F401

pytestmark = pytest.mark.gpu
L = _lib.lib


@pytest.fixture(autouse=True)
def det_mode():
    with ops.deterministic():
        yield


def p(t):
    return None if t is None else t.data_ptr()


def need_bytes():
    m = re.search(rb"needs (\d+) bytes", L().subgc_last_error())
    assert m, L().subgc_last_error()
    return int(m.group(1))


def ws(nbytes):
    return torch.empty(max(nbytes, 16) + 64, dtype=torch.uint8, device=DEV)


def shifted(t):
    """the same values at a 16-byte-aligned address + 4 bytes"""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


def stream():
    return torch.cuda.current_stream().cuda_stream


def sum_bound(terms_abs_sum):
    return 2e-6 * terms_abs_sum + 1e-30


# ---------------------------------------------------------------- embed_bwd
def embed_call(table, tok, keep, scale, dout, dtable, w, nbytes):
    n, E = dout.shape
    return L().subgc_embed_bwd_ws(p(table), p(tok), tok.stride(0), p(keep), ctypes.c_float(scale), p(dout), p(dtable), n, E, table.size(0), p(w), nbytes,
                                  stream())


def embed_ref(table, tok, keep, scale, dout, d0):
    g = dout.double().cpu()
    if keep is not None:
        g = g * keep.cpu().double() * scale
    out = d0.double().cpu().clone()
    out.index_add_(0, tok.cpu(), g)
    absum = torch.zeros_like(out).index_add_(0, tok.cpu(), g.abs())
    mask = table.cpu() > 0
    return torch.where(mask, out, d0.double().cpu()), absum


@pytest.mark.parametrize("kind", ["one_word", "zipf", "zipf_strided"])
def test_embed_bwd_repeats_and_is_accurate(kind):
    V, E, n = 1200, 320, 4000
    gen = torch.Generator().manual_seed(3)
    table = torch.randn(V, E, generator=gen).to(DEV)
    if kind == "one_word":
        tok = torch.full((n,), 7, dtype=torch.int64)
    else:
        z = torch.from_numpy(np.random.default_rng(4).zipf(1.3, n) - 1).clamp(max=V - 1)
        tok = torch.where(torch.rand(n, generator=gen) < 0.3, torch.zeros(n, dtype=torch.int64), z)      # pad rows
    tok = tok.to(DEV)
    if kind == "zipf_strided":                                   # a column of a [n, 3] token matrix (tok_stride 3)
        wide = torch.zeros(n, 3, dtype=torch.int64, device=DEV)
        wide[:, 1] = tok
        tok = wide[:, 1]
    keep = (torch.rand(n, E, generator=gen) > 0.5).to(torch.uint8).to(DEV)
    dout = torch.randn(n, E, generator=gen).to(DEV)
    d0 = torch.randn(V, E, generator=gen).to(DEV)
    assert embed_call(table, tok, keep, 2.0, dout, d0.clone(), None, 0) == -1
    need = need_bytes()
    assert embed_call(table, tok, keep, 2.0, dout, d0.clone(), ws(need), need - 4) == -1
    assert L().subgc_embed_bwd(p(table), p(tok), 1, p(keep), ctypes.c_float(2.0), p(dout), p(d0), n, E, V, stream()) == -1
    outs = []
    for i in range(20):
        d = d0.clone()
        w = ws(need if i % 2 else 64 << 20)
        assert embed_call(table, tok, keep, 2.0, dout if i < 10 else shifted(dout), d, w, need if i % 2 else (64 << 20)) == 0
        outs.append(d)
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    want, absum = embed_ref(table, tok, keep, 2.0, dout, d0)
    err = (outs[0].double().cpu() - want).abs()
    assert bool((err <= sum_bound(absum + d0.double().abs().cpu())).all()), float(err.max())


# ---------------------------------------------------------------- scatter_add_rows
@pytest.mark.parametrize("kind", ["one_row", "mixed"])
def test_scatter_add_rows_repeats_and_is_accurate(kind):
    M, Lc, R = 5000, 257, 300
    gen = torch.Generator().manual_seed(5)
    src = torch.randn(M, Lc, generator=gen).to(DEV)
    if kind == "one_row":
        rows = torch.full((M,), 11, dtype=torch.int32)
    else:
        rows = torch.randint(-1, R, (M,), generator=gen, dtype=torch.int32)
    rows = rows.to(DEV)
    m_dev = torch.tensor([M - 123], dtype=torch.int32, device=DEV)
    d0 = torch.randn(R, Lc, generator=gen).to(DEV)

    def call(s, d, w, nb):
        return L().subgc_scatter_add_rows_ws(p(s), Lc, p(rows), p(d), Lc, M, Lc, p(m_dev), R, p(w), nb, stream())

    assert call(src, d0.clone(), None, 0) == -1
    need = need_bytes()
    assert L().subgc_scatter_add_rows(p(src), Lc, p(rows), p(d0), Lc, M, Lc, p(m_dev), stream()) == -1
    outs = []
    for i in range(20):
        d = d0.clone()
        assert call(src if i < 10 else shifted(src), d, ws(need if i % 2 else 8 << 20), need if i % 2 else 8 << 20) == 0
        outs.append(d)
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    r = rows.cpu().long()[:M - 123]
    keep = r >= 0
    s = src.double().cpu()[:M - 123][keep]
    want = d0.double().cpu().index_add(0, r[keep], s)
    absum = d0.double().cpu().abs().index_add(0, r[keep], s.abs())
    assert bool(((outs[0].double().cpu() - want).abs() <= sum_bound(absum)).all())


# ---------------------------------------------------------------- sumsq
@pytest.mark.parametrize("n", [1, 1023, 4 * 1024 * 1024 + 3])
def test_sumsq_alignment_free_and_accurate(n):
    g = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(DEV)
    out0 = torch.tensor([1.5], device=DEV)
    assert L().subgc_sumsq_f32(p(g), n, p(out0), stream()) == -1
    assert L().subgc_sumsq_f32_ws(p(g), n, p(out0), None, 0, stream()) == -1
    need = need_bytes()
    res = []
    for i in range(20):
        o = out0.clone()
        x = g if i % 2 else shifted(g)
        nb = need if i % 4 < 2 else (1 << 20)
        assert L().subgc_sumsq_f32_ws(p(x), n, p(o), p(ws(nb)), nb, stream()) == 0
        res.append(o)
    for o in res[1:]:
        assert torch.equal(o, res[0])
    want = 1.5 + float((g.double().cpu() ** 2).sum())
    assert abs(float(res[0]) - want) <= 2e-6 * want


# ---------------------------------------------------------------- pool_bwd
def test_pool_bwd_every_subgraph_on_one_node():
    B, N, Lc, G = 4, 37, 300, 640
    gen = torch.Generator().manual_seed(9)
    idx = torch.randint(0, N, (G, N), generator=gen)
    idx[:, 0] = 5                                                   # every sub-graph holds node 5 of its image
    img = torch.zeros(G, dtype=torch.int32)                         # every sub-graph on image 0 (not grouped by image otherwise)
    img[G // 2:] = torch.randint(0, B, (G - G // 2,), generator=gen, dtype=torch.int32)
    w = (torch.rand(G, N, generator=gen) > 0.4).float()
    w[:, 0] = 1.0
    denom = w.sum(1).clamp(min=1)
    am = torch.randint(0, N, (G, Lc), generator=gen, dtype=torch.int32)
    dout = torch.randn(G, 2 * Lc, generator=gen)
    t = [x.to(DEV) for x in (idx, img, w, denom, am, dout)]
    idx_d, img_d, w_d, den_d, am_d, dout_d = t
    d0 = torch.randn(B * N, Lc, generator=gen).to(DEV)

    def call(d, wk, nb, dd=dout_d):
        return L().subgc_subgraph_pool_bwd_ws(p(dd), p(idx_d), N, p(w_d), N, 1, p(den_d), p(img_d), p(am_d), p(d), G, N, Lc, B * N, p(wk), nb, stream())

    assert call(d0.clone(), None, 0) == -1
    need = need_bytes()
    assert L().subgc_subgraph_pool_bwd(p(dout_d), p(idx_d), N, p(w_d), N, 1, p(den_d), p(img_d), p(am_d), p(d0), G, N, Lc, stream()) == -1
    assert b"subgc_subgraph_pool_bwd_ws" in L().subgc_last_error()
    with ops.deterministic(False):                                   # the mode-off (atomic) kernel, as a second reference
        atomic = d0.clone()
        assert call(atomic, None, 0) == 0
    outs = []
    for i in range(20):
        d = d0.clone()
        assert call(d, ws(need if i % 2 else 16 << 20), need if i % 2 else 16 << 20, dout_d if i < 10 else shifted(dout_d)) == 0
        outs.append(d)
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    want = d0.double().cpu().clone()
    absum = d0.double().cpu().abs()
    ii = torch.arange(N)
    for g in range(G):
        rows = int(img[g]) * N + idx[g]
        contrib = w[g].double()[:, None] * (dout[g, Lc:].double()[None, :] / float(denom[g]) +
                                             (am[g][None, :] == ii[:, None]).double() * dout[g, :Lc].double()[None, :])
        want.index_add_(0, rows, contrib)
        absum.index_add_(0, rows, contrib.abs())
    assert bool(((outs[0].double().cpu() - want).abs() <= 4e-6 * absum + 1e-12).all())
    assert bool(((outs[0].double().cpu() - atomic.double().cpu()).abs() <= 4e-6 * absum + 1e-12).all())


# ---------------------------------------------------------------- gpn_score_bwd
def test_score_bwd_2560x512():
    G, H = 2560, 512
    gen = torch.Generator().manual_seed(11)
    hid = torch.randn(G, H, generator=gen).to(DEV)
    keep = (torch.rand(G, H, generator=gen) > 0.5).to(torch.uint8).to(DEV)
    w2 = torch.randn(1, H, generator=gen).to(DEV)
    score = torch.rand(G, 1, generator=gen).clamp(0.05, 0.95).to(DEV)
    dloss = torch.ones((), device=DEV)

    def call(wk, nb):
        dhid, dw2, db2 = torch.empty_like(hid), torch.empty(1, H, device=DEV), torch.empty(1, device=DEV)
        rc = L().subgc_gpn_score_bwd_ws(p(hid), p(keep), ctypes.c_float(2.0), p(w2), p(score), p(dloss), p(dhid), p(dw2), p(db2), G, H, p(wk), nb, stream())
        return rc, dhid, dw2, db2

    assert call(None, 0)[0] == -1
    need = need_bytes()
    t = [torch.empty_like(hid), torch.empty(1, H, device=DEV), torch.empty(1, device=DEV)]
    assert L().subgc_gpn_score_bwd(p(hid), p(keep), ctypes.c_float(2.0), p(w2), p(score), p(dloss), p(t[0]), p(t[1]), p(t[2]), G, H, stream()) == -1
    assert b"subgc_gpn_score_bwd_ws" in L().subgc_last_error()
    runs = [call(ws(need if i % 2 else 1 << 22), need if i % 2 else 1 << 22) for i in range(20)]
    for r in runs:
        assert r[0] == 0
        for a, b in zip(r[1:], runs[0][1:]):
            assert torch.equal(a, b)
    s = score.double().cpu()[:, 0]
    t = (torch.arange(G) < G // 2).double()
    dz = (s - t) / ((1 - s) * s).clamp(min=1e-12) / G * (s * (1 - s))
    k = keep.cpu().double() * 2.0
    terms = dz[:, None] * hid.double().cpu() * k
    assert bool(((runs[0][2].double().cpu()[0] - terms.sum(0)).abs() <= 2e-6 * terms.abs().sum(0) + 1e-12).all())
    assert abs(float(runs[0][3]) - float(dz.sum())) <= 2e-6 * float(dz.abs().sum())


# ---------------------------------------------------------------- colsum
@pytest.mark.parametrize("M,N", [(700, 1), (64, 96), (5000, 1000), (3000, 7001)])
def test_colsum_alignment_and_workspace_free(M, N):
    x = torch.randn(M, N, generator=torch.Generator().manual_seed(M + N)).to(DEV)
    out0 = torch.randn(N, device=DEV)
    L().subgc_colsum_f32(p(x), N, M, N, p(out0), 1, None, None, 0, stream())
    need = need_bytes()
    res = []
    for i in range(8):
        o = out0.clone()
        xx = x if i % 2 else shifted(x)
        nb = need if i < 4 else 64 << 20
        assert L().subgc_colsum_f32(p(xx), N, M, N, p(o), 1, None, p(ws(nb)), nb, stream()) == 0
        res.append(o)
    for o in res[1:]:
        assert torch.equal(o, res[0])
    xb = x.to(torch.bfloat16)
    rb = []
    for i in range(4):
        o = out0.clone()
        xx = xb if i % 2 else shifted(xb)
        assert L().subgc_colsum_bf16(p(xx), N, M, N, p(o), 1, None, p(ws(need)), need, stream()) == 0
        rb.append(o)
    for o in rb[1:]:
        assert torch.equal(o, rb[0])
    want = out0.double().cpu() + x.double().cpu().sum(0)
    absum = out0.double().cpu().abs() + x.double().cpu().abs().sum(0)
    assert bool(((res[0].double().cpu() - want).abs() <= 2e-6 * absum).all())
    # m_dev (rows past it ignored) and accumulate = 0, at both alignments
    m_dev = torch.tensor([M - M // 3], dtype=torch.int32, device=DEV)
    rm = []
    for xx in (x, shifted(x)):
        o = torch.full((N,), 7.0, device=DEV)
        assert L().subgc_colsum_f32(p(xx), N, M, N, p(o), 0, p(m_dev), p(ws(need)), need, stream()) == 0
        rm.append(o)
    assert torch.equal(rm[0], rm[1])
    part = x.double().cpu()[:M - M // 3]
    assert bool(((rm[0].double().cpu() - part.sum(0)).abs() <= 2e-6 * part.abs().sum(0) + 1e-30).all())


# ---------------------------------------------------------------- two-pass BatchNorm
@pytest.mark.parametrize("M,C", [(3000, 256), (777, 250)])
def test_bn_fwd_bwd_alignment_and_workspace_free(M, C):
    gen = torch.Generator().manual_seed(M + C)
    X = (torch.randn(M, C, generator=gen) * 3 + 1).to(DEV)
    dY = torch.randn(M, C, generator=gen).to(DEV)
    gamma, beta = torch.randn(C, generator=gen).to(DEV), torch.randn(C, generator=gen).to(DEV)

    def fwd(x, wk, nb):
        y, sm, sr = torch.empty_like(x), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        rmean, rvar = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        rc = L().subgc_bn_fwd(p(x), p(y), M, C, p(gamma), p(beta), p(rmean), p(rvar), p(sm), p(sr), 1, ctypes.c_float(0.1), ctypes.c_float(1e-5),
                              p(wk), nb, stream())
        return rc, (y, sm, sr, rmean, rvar)

    def bwd(dy, x, sm, sr, wk, nb, shift_grads=False):
        dx, dg, db = torch.empty_like(x), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        if shift_grads:
            dg, db = shifted(dg), shifted(db)
        rc = L().subgc_bn_bwd(p(dy), p(x), p(gamma), p(sm), p(sr), p(dx), p(dg), p(db), M, C, p(wk), nb, stream())
        return rc, (dx, dg, db)

    assert fwd(X, ws(64), 16)[0] == -1
    need_f = need_bytes()
    res_f = []
    for i in range(6):
        nb = need_f if i % 2 else 32 << 20
        rc, out = fwd(X if i < 3 else shifted(X), ws(nb), nb)
        assert rc == 0
        res_f.append(out)
    for out in res_f[1:]:
        for a, b in zip(out, res_f[0]):
            assert torch.equal(a, b)
    y, sm, sr = res_f[0][:3]
    assert bwd(dY, X, sm, sr, ws(64), 16)[0] == -1
    need_b = need_bytes()
    res_b = []
    for i in range(6):
        nb = need_b if i % 2 else 32 << 20
        rc, out = bwd(dY if i < 3 else shifted(dY), X if i < 3 else shifted(X), sm, sr, ws(nb), nb, shift_grads=i >= 3)
        assert rc == 0
        res_b.append(out)
    for out in res_b[1:]:
        for a, b in zip(out, res_b[0]):
            assert torch.equal(a, b)
    x64, dy64 = X.double().cpu(), dY.double().cpu()
    mean = x64.mean(0)
    assert bool(((sm.double().cpu() - mean).abs() <= 2e-6 * x64.abs().mean(0)).all())
    var = ((x64 - mean) ** 2).mean(0)
    assert bool(((1.0 / sr.double().cpu() ** 2 - 1e-5 - var).abs() <= 1e-4 * var).all())
    xh = (x64 - sm.double().cpu()) * sr.double().cpu()
    dg_ref, db_ref = (dy64 * xh).sum(0), dy64.sum(0)
    assert bool(((res_b[0][1].double().cpu() - dg_ref).abs() <= 4e-6 * (dy64 * xh).abs().sum(0)).all())
    assert bool(((res_b[0][2].double().cpu() - db_ref).abs() <= 2e-6 * dy64.abs().sum(0)).all())


# ---------------------------------------------------------------- model level
def _train_run(make, batch, steps):
    """`steps` training iterations stepped the way bench.py steps them: reducer (world size 1), total loss, FlatAdam with zero_grad"""
    m = make()
    lw = models.LossWrapper(m, None)
    adam = parallel.FlatAdam(m, lr=5e-4)
    red = parallel.GradBucketReducer(m, optimizer=adam)
    b = {k: v.to(DEV) for k, v in batch.items()}
    losses = []
    for _ in range(steps):
        red.prepare()
        out = lw(b["fc_feats"], b["att_feats"], b["labels"], b["masks"], b["att_masks"], None, None, None, b["obj_dist"], None, b["rel_ind"],
                 None, b["pred_dist"], b["gpn_obj_ind"], b["gpn_pred_ind"], b["gpn_nrel_ind"], b["gpn_pool_mtx"])
        models.total_loss(out).backward()
        red.finish(average=False)
        adam.step(zero_grad=True)
        losses.append([float(out["lang_loss"].detach())] + ([float(out["gpn_loss"].detach())] if out.get("gpn_loss") is not None else []))
    torch.cuda.synchronize()
    st = {k: v.detach().clone() for k, v in m.state_dict().items() if "running_" in k}
    return losses, m.flat_params.detach().clone(), adam.m.clone(), adam.v.clone(), st


def _assert_runs_equal(a, b):
    assert a[0] == b[0]
    for x, y in zip(a[1:4], b[1:4]):
        assert torch.equal(x, y)
    assert a[4].keys() == b[4].keys()
    for k in a[4]:
        assert torch.equal(a[4][k], b[4][k]), k


@pytest.mark.parametrize("name,steps,over", [("subgc_train", 30, {}), ("fullgc_train", 30, {}), ("fullgc_train", 10, {"compute_dtype": "bf16"}),
                                             ("subgc_train", 5, {"sampling_prob": 0.25})])
def test_training_runs_repeat_bit_for_bit(golden, name, steps, over):
    g = golden(name)
    def make():
        m = models.setup(g.opt(**dict(dict(caption_model="topdown", drop_prob_lm=0.5, gpn_drop_prob=0.5), **over)))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in g.group("weights").items()})
        return m.to(DEV).train()
    torch.manual_seed(0)
    a = _train_run(make, g.tensors("inputs"), steps)
    torch.manual_seed(0)
    b = _train_run(make, g.tensors("inputs"), steps)
    _assert_runs_equal(a, b)


def test_bench_shape_repeats():
    from test_parity_gpu import KAR
    batch = synthetic.make_train_batch(128, seed=1)

    def make():
        torch.manual_seed(7)
        return models.setup(argparse.Namespace(**dict(KAR, drop_prob_lm=0.5, gpn_drop_prob=0.5))).to(DEV).train()
    a = _train_run(make, batch, 3)
    b = _train_run(make, batch, 3)
    _assert_runs_equal(a, b)


def test_forward_taps_repeat(golden):
    g = golden("subgc_train")
    m = build(g, g.group("weights"), True)
    b = {k: v.to(DEV) for k, v in g.tensors("inputs").items()}
    first = None
    for _ in range(50):
        m.tap = {}
        with torch.no_grad():
            m(*synthetic.forward_args(b))
        torch.cuda.synchronize()
        taps = {k: v.detach().clone() for k, v in m.tap.items() if torch.is_tensor(v)}
        if first is None:
            first = taps
            assert first
        else:
            assert taps.keys() == first.keys()
            for k in taps:
                assert torch.equal(taps[k], first[k]), k


@pytest.mark.parametrize("name", ["subgc_train", "subgc_gtsubg_train", "fullgc_train"])
def test_parity_with_goldens_in_mode(golden, name):
    g = golden(name)
    m = build(g, g.group("weights"), True)
    ref = g.group("out")
    out, loss = run_train(m, g.tensors("inputs"))
    close(out["lang_loss"], ref["lang_loss"], "lang_loss")
    if "gpn_loss" in ref:
        close(out["gpn_loss"], ref["gpn_loss"], "gpn_loss")
    grads, dead = g.group("grads"), set(g.meta["dead_params"])
    for k, prm in m.named_parameters():
        if k not in dead:
            close(prm.grad, grads[k], "grad " + k, atol=2e-4, rtol=2e-3)
