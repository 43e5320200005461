"""subgc_decode_sample (top-k sampling for any the_k, nucleus cut the_p) on the GPU: the kernel against a float64 restatement of its
rule on the same float32 logits, against subgc_decode_pick where both apply, its bookkeeping, and the model-level decode paths
(graphed loop, eager loop, two-image batch, bf16) against the oracle with injected uniforms.

Tolerances.  The order rule is exact (a stable descending sort of the float32 logits), so no tie is excluded anywhere.  A draw is
accepted when the uniform lies within delta of the float64 cdf interval of the kernel's token.  delta = 16 * d, where
d = max |cdf_float32 - cdf_float64| of a torch float32 restatement (log_softmax, exp, cumsum, divide) over ALL the kernel-test inputs
below: four bits over the reference arithmetic, for the device's expf / logf and a different summation order.  d is printed
(measured: 7.9e-7, delta = 1.3e-5).  seqlp: 1e-5 against the float64 tempered log-softmax (the tolerance of
test_decode_pick_greedy_topk_and_finished_masking).

Nucleus.  The prefix length m depends on the comparison c_j >= the_p of a summed mass with the_p.  Where the float64 mass stays
further than delta from the_p at the cut, m is determined and the window criterion runs over exactly those m tokens.  That
condition cannot hold in every row of every case by any choice of seed: at input scale 2 the tempered row is flat, the token at the
0.99 cut carries a mass of ~1.2e-5 ~ delta, and 898 of 900 rows have a summed mass within delta of 0.99 (0.9: ~10 %).  So no row
is skipped; instead every prefix length m' admissible under the same delta (c[m'-1] >= the_p - delta and c[m'-2] < the_p + delta)
is allowed, and the window criterion must hold for one of them -- for a row that meets the margin condition this IS the exact
criterion.  The cases in CLEAN (checked on the CPU for the seeds below) meet the margin condition in every row, and that is
asserted.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import subgc_oracle as O
from subgc import ops, synthetic
from subgc.models import sampling
import subgc.models as models

from test_sample_pick_cpu import topk10_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V, TEMP = 9488, 0.6
TEMP32 = float(np.float32(TEMP))                                                # what the kernel divides by
SEEDS = {(2.0, 64): 100, (2.0, 900): 100, (6.0, 64): 100, (6.0, 900): 102}
KS = (9, 16, 64, 1000, 9488)
# (scale, n, the_p, k) whose float64 prefix mass keeps a margin > delta from the_p at the cut in EVERY row
CLEAN = ({(6.0, 64, p, k) for p in (0.5, 0.9, 0.99) for k in (9488, 20)} | {(2.0, n, 0.5, k) for n in (64, 900) for k in (9488, 20)}
         | {(2.0, n, p, 20) for n in (64, 900) for p in (0.9, 0.99)} | {(6.0, 900, p, k) for p in (0.5, 0.9) for k in (9488, 20)})


@functools.lru_cache(None)
def inputs(scale, n):
    """-> x [n, V] float32, u [n] (fixed seed + the edge values), order (stable descending sort of x), vs (float64 tempered
    log-softmax in that order), v32 (the same in torch float32)."""
    g = torch.Generator().manual_seed(SEEDS[(scale, n)])
    x = (torch.randn(n, V, generator=g) * scale).float()
    u = torch.rand(n, generator=g)
    u[0], u[1] = 0.0, 1.0 - 2.0 ** -24
    order = torch.sort(x, dim=1, descending=True, stable=True).indices
    vs = torch.log_softmax(x.double() / TEMP32, 1).gather(1, order)
    v32 = torch.log_softmax(x / np.float32(TEMP), 1).gather(1, order)
    return x, u, order, vs, v32


@functools.lru_cache(None)
def delta():
    d = 0.0
    for (scale, n) in SEEDS:
        _, _, _, vs, v32 = inputs(scale, n)
        c64 = vs.exp().cumsum(1)
        for k in KS:
            c32 = v32[:, :k].exp().cumsum(1)
            d = max(d, float(((c32 / c32[:, -1:]).double() - c64[:, :k] / c64[:, k - 1:k]).abs().max()))
    print(f"d = max |cdf_float32 - cdf_float64| = {d:.3e}, delta = {16 * d:.3e}")
    assert 1e-8 < d < 5e-6
    return 16 * d


def buffers(n, T=4):
    z = lambda *s, dt: torch.zeros(*s, dtype=dt, device=DEV)
    return z(n, T, dt=torch.long), z(n, T, dt=torch.float32), z(n, dt=torch.long), z(n, dt=torch.int32), z(T, dt=torch.int32)


def run_new(x, u, k, top_p=1.0):
    seq, slp, it, unf, cnt = buffers(x.size(0))
    ops.decode_sample(x.to(DEV), k, top_p, TEMP, None if u is None else u.to(DEV), 0, seq, slp, it, unf, cnt[0:1], None, raw=True)
    torch.cuda.synchronize()
    return seq[:, 0].cpu(), slp[:, 0].cpu()


def check_window(tok, lp, u, order, vs, k, top_p, dl):
    """Every row: the token is one of the kept prefix, u lies within dl of its float64 cdf interval, lp is its tempered log-prob.
    -> number of rows whose prefix length is not determined within dl (0 when top_p == 1)."""
    n = tok.numel()
    ck = vs[:, :k].exp().cumsum(1)
    hit = order[:, :k] == tok.view(-1, 1)
    assert bool(hit.any(1).all()), "a token outside the k leading logits"
    pos = hit.float().argmax(1)
    first = lambda thr: torch.where((ck >= thr).any(1), (ck >= thr).float().argmax(1) + 1, torch.tensor(k))
    lo_m, hi_m = (first(top_p - dl), first(top_p + dl)) if top_p < 1.0 else (torch.full((n,), k), torch.full((n,), k))
    ud = u.double()
    ok = torch.zeros(n, dtype=torch.bool)
    for dm in range(int((hi_m - lo_m).max()) + 1):
        m = torch.minimum(lo_m + dm, hi_m)
        z = ck.gather(1, (m - 1).view(-1, 1)).view(-1)
        upper = ck.gather(1, pos.view(-1, 1)).view(-1) / z
        lower = torch.where(pos > 0, ck.gather(1, (pos - 1).clamp(min=0).view(-1, 1)).view(-1) / z, torch.zeros(n, dtype=torch.float64))
        ok |= (pos < m) & (lower - dl <= ud) & ((ud < upper + dl) | (pos == m - 1))
    assert bool(ok.all()), (int((~ok).sum()), (~ok).nonzero().flatten()[:8].tolist())
    want_lp = vs.gather(1, pos.view(-1, 1)).view(-1)
    assert float((lp.double() - want_lp).abs().max()) < 1e-5, float((lp.double() - want_lp).abs().max())
    return int((lo_m != hi_m).sum())


# ---------------------------------------------------------------------------------------------------------------- 3. kernel vs float64
@pytest.mark.parametrize("scale,n", list(SEEDS))
def test_kernel_against_float64_restatement(scale, n):
    x, u, order, vs, _ = inputs(scale, n)
    dl = delta()
    for k in KS:
        tok, lp = run_new(x, u, k)
        assert check_window(tok, lp, u, order, vs, k, 1.0, dl) == 0
        # u = 0 takes the largest logit, u = 1 - 2^-24 a token whose cdf interval reaches up to it
        assert int(tok[0]) == int(order[0, 0])


# ---------------------------------------------------------------------------------------------------------------- 4. old vs new kernel
@pytest.mark.parametrize("scale,n", list(SEEDS))
def test_old_and_new_kernel_agree_for_small_k(scale, n):
    x, u, order, vs, _ = inputs(scale, n)
    dl = delta()
    exempt = total = 0
    for k in (1, 3, 8):
        tok, lp = run_new(x, u, k)
        seq, slp, it, unf, cnt = buffers(n)
        ops.decode_pick(x.to(DEV), k, TEMP, u.to(DEV), 0, seq, slp, it, unf, cnt[0:1], None, raw=True)        # k <= 8: subgc_decode_pick
        ck = vs[:, :k].exp().cumsum(1)
        cdf = ck / ck[:, -1:]
        far = ((cdf[:, :-1] - u.double().view(-1, 1)).abs() > dl).all(1) if k > 1 else torch.ones(n, dtype=torch.bool)
        assert torch.equal(tok[far], seq[:, 0].cpu()[far])
        assert float((lp[far] - slp[:, 0].cpu()[far]).abs().max()) < 1e-5
        exempt += int((~far).sum()); total += n
    assert exempt <= 0.01 * total, (exempt, total)


# ---------------------------------------------------------------------------------------------------------------- 5. nucleus
@pytest.mark.parametrize("scale,n", list(SEEDS))
def test_nucleus_against_float64_restatement(scale, n):
    x, u, order, vs, _ = inputs(scale, n)
    dl = delta()
    for top_p in (0.5, 0.9, 0.99):
        for k in (9488, 20):
            tok, lp = run_new(x, u, k, top_p)
            undetermined = check_window(tok, lp, u, order, vs, k, top_p, dl)
            print(f"scale {scale} n {n} the_p {top_p} k {k}: {undetermined} rows within delta of the cut")
            if (scale, n, top_p, k) in CLEAN:
                assert undetermined == 0
    # top_p = 1 is plain top-k, bit for bit
    for k in (20, 9488):
        a, b = run_new(x, u, k, 1.0), run_new(x, u, k)
        seq, slp, it, unf, cnt = buffers(n)
        ops.decode_pick(x.to(DEV), k, TEMP, u.to(DEV), 0, seq, slp, it, unf, cnt[0:1], None, raw=True, top_p=1.0)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], seq[:, 0].cpu()) and torch.equal(a[1], slp[:, 0].cpu())
    # a mass so small that one token is kept: the arg-max, with its tempered log-prob
    for k in (20, 9488):
        tok, lp = run_new(x, u, k, 1e-6)
        assert torch.equal(tok, order[:, 0])
        assert float((lp.double() - vs[:, 0]).abs().max()) < 1e-5


# ---------------------------------------------------------------------------------------------------------------- 6. bookkeeping
def test_bookkeeping_finished_masking_flag_and_early_break():
    n, T, k = 6, 20, 20
    x = (torch.randn(n, V, generator=torch.Generator().manual_seed(3)) * 2.0).float()
    x[2, 0] = 12.0                                                      # row 2 emits <eos> at t = 0: p(<eos>) = 0.995 > its uniform 0.5
    xd = x.to(DEV)
    u = torch.tensor([0.0, 0.3, 0.5, 0.7, 0.95, 0.999], device=DEV)
    seq, slp, it, unf, cnt = buffers(n, T)
    ops.decode_sample(xd, k, 1.0, TEMP, u, 0, seq, slp, it, unf, cnt[0:1], None)
    order = torch.sort(x, dim=1, descending=True, stable=True).indices
    vs = torch.log_softmax(x.double() / TEMP32, 1).gather(1, order)
    check_window(seq[:, 0].cpu(), slp[:, 0].cpu(), u.cpu(), order, vs, k, 1.0, delta())       # at t = 0 seq holds the drawn word itself
    w = seq[:, 0].cpu()
    assert int(w[2]) == 0 and int(unf[2]) == 0 and torch.equal(unf.cpu(), (w > 0).int()) and torch.equal(it.cpu(), w)
    assert (int(cnt[0]) != 0) == bool((w > 0).any()) and int(cnt[0]) != 0
    first = (seq.clone(), slp.clone(), it.clone(), unf.clone())
    # step 1: the finished row stays finished although it would pick a word; its seqlp is still written (un-masked)
    ops.decode_sample(xd.roll(1, 1).contiguous(), k, 1.0, TEMP, u, 1, seq, slp, it, unf, cnt[1:2], cnt[0:1])
    assert int(seq[2, 1]) == 0 and int(unf[2]) == 0 and float(slp[2, 1]) != 0.0 and int(it[2]) == 0
    assert bool((seq[:, 1].cpu()[[0, 1, 3, 4, 5]] > 0).all())
    # every row finished: the flag stays zero
    eos = torch.full((n, V), -5.0); eos[:, 0] = 50.0
    s2, l2, i2, f2, c2 = buffers(n, T)
    ops.decode_sample(eos.to(DEV), k, 1.0, TEMP, u, 0, s2, l2, i2, f2, c2[0:1], None)
    assert int(c2[0]) == 0 and int(f2.sum()) == 0 and int(s2.abs().sum()) == 0
    # device-side early break: prev_count == 0 writes nothing
    before = (seq.clone(), slp.clone(), it.clone(), unf.clone(), cnt.clone())
    ops.decode_sample(xd, k, 1.0, TEMP, u, 5, seq, slp, it, unf, cnt[5:6], c2[0:1])
    for a, b in zip(before, (seq, slp, it, unf, cnt)):
        assert torch.equal(a, b)
    # two launches on the same inputs: identical bits (also with a nucleus cut)
    for top_p in (1.0, 0.9):
        outs = []
        for _ in range(2):
            s3, l3, i3, f3, c3 = buffers(n, T)
            ops.decode_sample(xd, k, top_p, TEMP, u, 0, s3, l3, i3, f3, c3[0:1], None)
            outs.append((s3, l3, i3, f3, c3))
        for a, b in zip(*outs):
            assert torch.equal(a, b)
        if top_p == 1.0:
            assert torch.equal(outs[0][0], first[0]) and torch.equal(outs[0][1], first[1])
    # limits are checked on the host
    for bad in (dict(k=0), dict(k=V + 1), dict(top_p=0.0), dict(top_p=1.5)):
        with pytest.raises(Exception, match="decode_sample"):
            ops.decode_sample(xd, bad.get("k", k), bad.get("top_p", 1.0), TEMP, u, 0, seq, slp, it, unf, cnt[0:1], None)


# ---------------------------------------------------------------------------------------------------------------- 7. model level
def build(g, weights, **over):
    m = models.setup(g.opt(caption_model="topdown", gpn_drop_prob=0.0, **over))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    return m.to(DEV).eval()


def upto_eos(seq):
    alive = torch.ones_like(seq, dtype=torch.bool)
    alive[:, 1:] = (seq[:, :-1] > 0).cumprod(1).bool()
    return alive


def oracle_margin(tap, seq, u):
    """Smallest distance of a live draw's uniform from a boundary of the oracle's float64 cdf, and whether two top-k log-probs tie."""
    live = upto_eos(seq)
    best, tie = 1.0, False
    for t in range(len(tap["topk_lp"])):
        top = tap["topk_lp"][t].double()
        cdf = torch.softmax(top, 1).cumsum(1)[:, :-1]
        rows = live[:, t]
        if cdf.size(1) and bool(rows.any()):
            best = min(best, float((cdf[rows] - u[rows, t].double().view(-1, 1)).abs().min()))
            tie |= bool((top[rows, 1:] == top[rows, :-1]).any())
    return best, tie


def product_paths(g, w, b, sopt, u, **over):
    """(name, result tuple) for the graphed loop, the eager loop and both images of a two-image batch."""
    args = synthetic.sample_args(b)
    m = build(g, w, **over)
    yield "graphed", m(*args, opt=sopt, mode="sample", uniforms=u.to(DEV))
    assert [x for x in m._graph_cache.values() if hasattr(x, "st")], "the graphed loop did not run"
    m = build(g, w, **over)
    m.decode_hipgraph = False
    yield "eager", m(*args, opt=sopt, mode="sample", uniforms=u.to(DEV))
    m = build(g, w, **over)
    images = [b, b]
    att, obj, pred, rel = ops.stack_first([[im[k] for im in images] for k in ("att_feats", "obj_dist", "pred_dist", "rel_ind")])
    I, N, _ = att.shape
    X2 = m._encode(att, obj, pred, rel).reshape(I * N, m.GCN_dim).contiguous()
    rows = [(i, im["gpn_obj_ind"], im["att_masks"], im["gpn_pool_mtx"]) for i, im in enumerate(images)]
    rets = sampling.decode(m, X2, N, sampling.select_subgraphs(m, X2, N, rows), sopt, uniforms=torch.cat([u, u]).to(DEV))
    assert len(rets) == 2
    for i, r in enumerate(rets):
        yield f"batch[{i}]", r


def topk_case(golden):
    g = golden("subgc_topk")
    return g, golden("subgc_train").group("weights"), g.tensors("inputs"), g.meta["sample_opt"]


@pytest.mark.parametrize("k,seed", [(9, 12), (10, 12), (10, 13), (51, 12)])
def test_model_sampling_equals_the_oracle_with_injected_uniforms(golden, k, seed):
    g, w, tb, sopt = topk_case(golden)
    n, T = g.group("out")["seq"].shape
    u = torch.rand(n, T, generator=torch.Generator().manual_seed(seed))
    tap = {}
    want = O.Oracle(g.opt(the_k=k), w).sample(*synthetic.sample_args(tb), opt=sopt, uniforms=u, tap=tap)
    margin, tie = oracle_margin(tap, want[0], u)
    print(f"the_k {k} seed {seed}: min distance of a uniform from an oracle cdf boundary {margin:.2e}")
    assert margin >= 1e-4 and not tie
    b = {kk: v.to(DEV) for kk, v in tb.items()}
    for name, ret in product_paths(g, w, b, sopt, u, the_k=k):
        np.testing.assert_array_equal(ret[3].cpu().numpy(), want[3].numpy(), err_msg=name)
        np.testing.assert_array_equal(ret[0].cpu().numpy(), want[0].numpy(), err_msg=name)
        np.testing.assert_allclose(ret[1].cpu().numpy(), want[1].numpy(), atol=2e-4, rtol=1e-4, err_msg=name)


@pytest.mark.parametrize("k,seed", [(25, 11), (51, 13)])
def test_model_sampling_window_criterion_along_its_own_path(golden, k, seed):
    """Pairs whose uniforms come closer than 1e-4 to an oracle cdf boundary: the oracle is forced with the product's tokens; every live
    token lies in its tapped top-k, the log-probs agree within 2e-4 and u lies within 2e-4 of the token's float64 cdf interval (a
    log-prob error eps moves a renormalised cdf by at most 2 eps; eps = the 1e-4 fp32 tolerance)."""
    g, w, tb, sopt = topk_case(golden)
    n, T = g.group("out")["seq"].shape
    u = torch.rand(n, T, generator=torch.Generator().manual_seed(seed))
    b = {kk: v.to(DEV) for kk, v in tb.items()}
    orc = O.Oracle(g.opt(the_k=k), w)
    for name, ret in product_paths(g, w, b, sopt, u, the_k=k):
        seq = ret[0].cpu()
        tap = {}
        forced = orc.sample(*synthetic.sample_args(tb), opt=sopt, forced=seq, tap=tap)
        np.testing.assert_array_equal(ret[3].cpu().numpy(), forced[3].numpy(), err_msg=name)
        live = upto_eos(seq)
        np.testing.assert_allclose(ret[1].cpu()[live].numpy(), forced[1][live].numpy(), atol=2e-4, rtol=0, err_msg=name)
        checked = 0
        for t in range(len(tap["topk_lp"])):
            cdf = torch.softmax(tap["topk_lp"][t].double(), 1).cumsum(1)
            for r in live[:, t].nonzero().flatten().tolist():
                tok = int(seq[r, t])                                   # a live row shows the drawn word itself (0: <eos> was drawn)
                idx = tap["topk_idx"][t][r].tolist()
                assert tok in idx, (name, r, t)
                j = idx.index(tok)
                lo = float(cdf[r, j - 1]) if j else 0.0
                assert lo - 2e-4 <= float(u[r, t]) and (float(u[r, t]) < float(cdf[r, j]) + 2e-4 or j == k - 1), (name, r, t, j)
                checked += 1
        assert checked > 50


def test_model_bf16_sampling_forks_are_explained(golden):
    """compute_dtype = bf16 at the_k = 10 under the criterion of test_bf16_topk_sampling_with_injected_uniforms_follows_the_oracle: a
    fork from the fp32 oracle is explained at its first differing step by a uniform within 5e-2 of a cdf boundary between the two
    words, or by two top-k words whose tempered log-probs lie within 2 * 5e-2 / temp."""
    g, w, tb, sopt = topk_case(golden)
    k = 10
    n, T = g.group("out")["seq"].shape
    u = torch.rand(n, T, generator=torch.Generator().manual_seed(12))
    m = build(g, w, the_k=k, compute_dtype="bf16")
    ret = m(*synthetic.sample_args({kk: v.to(DEV) for kk, v in tb.items()}), opt=sopt, mode="sample", uniforms=u.to(DEV))
    orc = O.Oracle(g.opt(the_k=k), w)
    tap = {}
    want = orc.sample(*synthetic.sample_args(tb), opt=sopt, uniforms=u, tap=tap)
    forced = orc.sample(*synthetic.sample_args(tb), opt=sopt, forced=ret[0].cpu())
    np.testing.assert_array_equal(ret[3].cpu().numpy(), want[3].numpy())
    got = ret[0].cpu()
    live = upto_eos(got)
    np.testing.assert_allclose(ret[1].cpu()[live].numpy(), forced[1][live].numpy(), atol=5e-2, rtol=0)
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


def test_model_on_the_reference_path_at_k10(golden):
    """The product forced along the reference's sampled path of subgc_topk10: kept sub-graphs identical, log-probs within 2e-4."""
    g = topk10_case(golden)
    ref = g.group("out")
    m = build(g, golden("subgc_train").group("weights"))
    assert m.the_k == 10
    b = {k: v.to(DEV) for k, v in g.tensors("inputs").items()}
    ret = m(*synthetic.sample_args(b), opt=g.meta["sample_opt"], mode="sample", forced=torch.from_numpy(ref["seq"]).to(DEV))
    np.testing.assert_array_equal(ret[3].cpu().numpy(), ref["keep_ind"])
    alive = np.ones(ref["seq"].shape[0], bool)
    ours = ret[1].cpu().numpy()
    for t in range(ref["seq"].shape[1]):
        sel = alive & (ref["seq"][:, t] > 0)
        np.testing.assert_allclose(ours[sel, t], ref["seqLogprobs"][sel, t], atol=2e-4)
        alive &= ref["seq"][:, t] > 0


# ---------------------------------------------------------------------------------------------------------------- 8. free-running
@pytest.mark.parametrize("over", [dict(the_k=20), dict(the_k=20, the_p=0.9)])
def test_free_running_decode_is_reproducible(golden, over):
    g, w, tb, sopt = topk_case(golden)
    args = synthetic.sample_args({k: v.to(DEV) for k, v in tb.items()})
    runs = []
    for _ in range(2):
        m = build(g, w, **over)
        torch.manual_seed(77)
        runs.append([m(*args, opt=sopt, mode="sample") for _ in range(2)] + list(m.sample_images([{k: v.to(DEV) for k, v in tb.items()}] * 2, opt=sopt)))
    for a, b in zip(*runs):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    assert not torch.equal(runs[0][0][0], runs[0][1][0])                       # the call counter moves the stream


def test_whole_vocabulary_sampling_is_wider_than_top3(golden):
    """A sanity check that the wide path is taken, not a statistic: over 200 rows the first word of the_k = vocab_size + 1 takes more
    than the three values the_k = 3 can give a row."""
    g, w, tb, sopt = topk_case(golden)
    args = synthetic.sample_args({k: v.to(DEV) for k, v in tb.items()})
    distinct = {}
    for k in (3, 51):
        m = build(g, w, the_k=k)
        torch.manual_seed(5)
        first = torch.stack([m(*args, opt=sopt, mode="sample")[0][:, 0].cpu() for _ in range(20)])          # [20 images, 10 rows]
        assert first.numel() == 200
        distinct[k] = max(len(set(first[:, r].tolist())) for r in range(first.size(1)))
    assert distinct[3] <= 3 < distinct[51], distinct
