"""subgc.optim on the MI355X: every `--optim` rule of build_optimizer (misc/utils.py:223-239) as one fused clip + update sweep
(subgc_clip_optim_step), against torch.optim driving the oracle's parameters in the reference's order with the reference's global-norm
clip (misc/utils.py:174-200); the warm-up schedule of train.py:107-124 through param_groups; checkpoint resume fused -> fused (bit for
bit), torch -> fused and fused -> torch; and the plumbing: bf16 snapshot, GradBucketReducer, the zero_grad fold, no ATen kernels."""
import argparse
import collections
import io
import math

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from oracle import subgc_oracle as O
import subgc.models as models
from subgc import ops, optim, parallel, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATOL, PRTOL = 2e-5, 1e-3

# (opt.optim, learning rate, opt.weight_decay, clip norm): the SGD family runs at a large rate so that its decay terms show; the cases
# with clip 2 have the clip active (the golden batch's gradient norm is about 8.3)
CASES = [("adam", 5e-4, 0.0, 2.0), ("adamw", 1e-3, 0.0, 10.0), ("sgd", 5e-2, 0.0, 10.0), ("sgdm", 5e-2, 1e-3, 2.0),
         ("sgdmom", 5e-2, 0.0, 10.0), ("rmsprop", 1e-3, 1e-3, 10.0), ("adagrad", 1e-2, 1e-3, 10.0)]
RULES = [c[0] for c in CASES]


def close(a, b, name, atol=1e-4, rtol=1e-4):
    a = a.detach().float().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().float().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    np.testing.assert_allclose(a, b, atol=atol, rtol=rtol, err_msg=name)


def build(g, weights, train, **over):
    m = models.setup(g.opt(caption_model="topdown", gpn_drop_prob=0.0, **over))
    m.load_state_dict({k: torch.as_tensor(v) for k, v in weights.items()})
    m = m.to(DEV)
    m.train(train)
    return m


def ns(rule, lr, wd):
    return argparse.Namespace(optim=rule, learning_rate=lr, optim_alpha=0.9, optim_beta=0.999, optim_epsilon=1e-8, weight_decay=wd)


def torch_optimizer(params, o):
    """The torch class misc/utils.py:223-239 constructs for `o.optim`, over `params`."""
    return {"rmsprop": lambda: torch.optim.RMSprop(params, o.learning_rate, o.optim_alpha, o.optim_epsilon, weight_decay=o.weight_decay),
            "adagrad": lambda: torch.optim.Adagrad(params, o.learning_rate, weight_decay=o.weight_decay),
            "sgd": lambda: torch.optim.SGD(params, o.learning_rate, weight_decay=5e-4, momentum=0.9),
            "sgdm": lambda: torch.optim.SGD(params, o.learning_rate, o.optim_alpha, weight_decay=o.weight_decay),
            "sgdmom": lambda: torch.optim.SGD(params, o.learning_rate, o.optim_alpha, weight_decay=o.weight_decay, nesterov=True),
            "adam": lambda: torch.optim.Adam(params, o.learning_rate, (o.optim_alpha, o.optim_beta), o.optim_epsilon, weight_decay=o.weight_decay),
            "adamw": lambda: torch.optim.AdamW(params, o.learning_rate, weight_decay=0.01)}[o.optim]()


class TorchSide:
    """The oracle's parameters (reference order) driven by torch.optim with the reference's clip: train.py:150-164."""

    def __init__(self, g, weights, o, clip):
        self.orc = O.Oracle(g.opt(gpn_drop_prob=0.0), weights, requires_grad=True)
        self.orc.training = True
        self.params = list(self.orc.P.values())
        self.opt = torch_optimizer(self.params, o)
        self.clip, self.norms = clip, []

    def step(self, batch):
        self.opt.zero_grad()
        ref = O.loss_wrapper(self.orc, batch)
        loss = ref["lang_loss"] + ref["gpn_loss"]
        loss.backward()
        total = math.sqrt(sum(float(p.grad.norm(2)) ** 2 for p in self.params if p.grad is not None))    # misc/utils.py:189-191
        coef = self.clip / max(total, self.clip)                                                              # :193
        for p in self.params:
            if p.grad is not None:
                p.grad.mul_(coef)
        self.opt.step()
        self.norms.append(total)
        return float(loss.detach())


def fused_step(m, fopt, batch):
    fopt.zero_grad()
    b = {k: v.to(DEV) for k, v in batch.items()}
    out = models.LossWrapper(m, None)(b["fc_feats"], b["att_feats"], b["labels"], b["masks"], b["att_masks"], None, None, None, b["obj_dist"],
                                      None, b["rel_ind"], None, b["pred_dist"], b["gpn_obj_ind"], b["gpn_pred_ind"], b["gpn_nrel_ind"],
                                      b["gpn_pool_mtx"])
    loss = out["lang_loss"] + out["gpn_loss"]
    loss.backward()
    fopt.step()
    return float(loss.detach())


# the attention softmax is invariant to a shift of its scores, so alpha_net.bias has a gradient of zero in exact arithmetic: what
# either side computes is rounding noise, which the adaptive rules (Adam, AdamW, RMSprop, Adagrad) normalise into steps of about
# +-lr in a direction that depends on the summation order -- the two trajectories of that one scalar are not comparable there
NOISE_ONLY = "core.attention.alpha_net.bias"
ADAPTIVE = ("adam", "adamw", "rmsprop", "adagrad")


def compare_params(m, orc, what, rule):
    for k, p in orc.P.items():
        if k == NOISE_ONLY and rule in ADAPTIVE:
            continue
        close(m.P(k), p, f"{what}: param {k}", atol=PATOL, rtol=PRTOL)


def weights_of(m):
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


# ------------------------------------------------------------------------------------------------ the sweep itself
TORCH_SINGLE = {"adam": lambda p: torch.optim.Adam(p, 1e-2, (0.8, 0.99), 1e-6, weight_decay=0.1, foreach=False),
                "adamw": lambda p: torch.optim.AdamW(p, 1e-2, (0.8, 0.99), 1e-6, weight_decay=0.1, foreach=False),
                "sgd": lambda p: torch.optim.SGD(p, 0.1, momentum=0.9, dampening=0.25, weight_decay=0.1, foreach=False),
                "sgdmom": lambda p: torch.optim.SGD(p, 0.1, momentum=0.9, weight_decay=0.1, nesterov=True, foreach=False),
                "sgd0": lambda p: torch.optim.SGD(p, 0.1, weight_decay=0.1, foreach=False),
                "rmsprop": lambda p: torch.optim.RMSprop(p, 1e-2, 0.9, 1e-6, weight_decay=0.1, foreach=False),
                "adagrad": lambda p: torch.optim.Adagrad(p, 1e-1, lr_decay=0.05, weight_decay=0.1, foreach=False)}


@pytest.mark.parametrize("zero", [False, True])
@pytest.mark.parametrize("n", [4096, 4099])
@pytest.mark.parametrize("kind", list(TORCH_SINGLE))
def test_sweep_matches_torch_single_tensor_with_skipped_ranges(kind, n, zero):
    """Three clipped steps on random data: the live ranges (bounds off the float4 grid) follow torch's single-tensor update of the same
    parameters, with strong decay and non-default hyperparameters; the skipped ranges keep weight, state and (unless zeroed) gradient
    bit for bit.  n = 4099: the scalar form."""
    gen = torch.Generator().manual_seed(n + 7)
    bounds = [5, 1001, 1003, 2050, 3000, n]
    live = [(bounds[i], bounds[i + 1]) for i in range(0, len(bounds), 2)]
    p0 = torch.randn(n, generator=gen)
    ref = [torch.nn.Parameter(p0[lo:hi].clone()) for lo, hi in live]
    topt = TORCH_SINGLE[kind](ref)
    g0 = topt.param_groups[0]
    p = p0.clone().to(DEV)
    gbuf = torch.zeros(n, device=DEV)
    s1, s2 = torch.rand(n, device=DEV), torch.rand(n, device=DEV)          # the skipped ranges' state must survive untouched
    for lo, hi in live:
        s1[lo:hi] = 0.0
        s2[lo:hi] = 0.0
    keep = (s1.clone(), s2.clone())
    table = torch.tensor(bounds, dtype=torch.int64, device=DEV)
    sumsq = torch.zeros(1, device=DEV)
    rule = {"sgd0": "sgd", "sgdmom": "sgd"}.get(kind, kind)
    for t in range(1, 4):
        grads = [torch.randn(hi - lo, generator=gen) * 3.0 for lo, hi in live]
        gbuf.zero_()
        for (lo, hi), gr in zip(live, grads):
            gbuf[lo:hi] = gr.to(DEV)
        total = math.sqrt(sum(float(gr.norm()) ** 2 for gr in grads))
        coef = 4.0 / max(total, 4.0)
        assert coef < 1.0
        for r, gr in zip(ref, grads):
            r.grad = gr * coef
        topt.step()
        ops.fill_(sumsq, 0.0)
        ops.sumsq(gbuf, sumsq)
        if rule in ("adam", "adamw"):
            h0, h1, eps = g0["betas"][0], g0["betas"][1], g0["eps"]
        elif rule == "sgd":
            h0, h1, eps = g0["momentum"], g0["dampening"], 0.0
        elif rule == "rmsprop":
            h0, h1, eps = g0["alpha"], 0.0, g0["eps"]
        else:
            h0, h1, eps = g0["lr_decay"], 0.0, g0["eps"]
        ops.clip_optim_step(rule, p, gbuf, s1, s2 if rule in ("adam", "adamw") else None, table, sumsq, 4.0, 1.0, g0["lr"], h0, h1, eps,
                            g0["weight_decay"], t, nesterov=g0.get("nesterov", False), first=t == 1, zero_grad=zero)
        torch.cuda.synchronize()
        for (lo, hi), r, gr in zip(live, ref, grads):
            close(p[lo:hi], r, f"{kind} step {t} p[{lo}:{hi}]", atol=1e-6, rtol=1e-5)
            close(gbuf[lo:hi], torch.zeros_like(gr) if zero else gr * coef, "gradient after the sweep", atol=1e-7, rtol=1e-6)
        dead = torch.ones(n, dtype=torch.bool)
        for lo, hi in live:
            dead[lo:hi] = False
        assert torch.equal(p.cpu()[dead], p0[dead])
        assert torch.equal(s1.cpu()[dead], keep[0].cpu()[dead]) and torch.equal(s2.cpu()[dead], keep[1].cpu()[dead])
    st = topt.state_dict()["state"]
    key = {"adam": "exp_avg", "adamw": "exp_avg", "rmsprop": "square_avg", "adagrad": "sum"}.get(rule, "momentum_buffer")
    if kind != "sgd0":
        for i, (lo, hi) in enumerate(live):
            close(s1[lo:hi], st[i][key], f"{kind} state {key}", atol=1e-6, rtol=1e-5)


def _whole_bucket_against_full_table(n, zero, wd):
    gen = torch.Generator().manual_seed(3)
    p = torch.randn(n, generator=gen).to(DEV)
    a = [p.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    b = [p.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    sa, sb = torch.empty(n, device=DEV, dtype=torch.bfloat16), torch.empty(n, device=DEV, dtype=torch.bfloat16)
    ss = torch.zeros(1, device=DEV)
    table = torch.tensor([0, n], dtype=torch.int64, device=DEV)
    for t in range(1, 4):
        g = (torch.randn(n, generator=gen) * 0.1).to(DEV)
        ops.fill_(ss, 0.0)
        ops.sumsq(g, ss)
        ga, gb = g.clone(), g.clone()
        ops.clip_optim_step("adam", a[0], ga, a[1], a[2], None, ss, 10.0, 1.0, 1e-3, 0.9, 0.999, 1e-8, wd, t, p_bf16=sa, zero_grad=zero)
        ops.clip_optim_step("adam", b[0], gb, b[1], b[2], table, ss, 10.0, 1.0, 1e-3, 0.9, 0.999, 1e-8, wd, t, p_bf16=sb, zero_grad=zero)
        assert torch.equal(ga, gb) and (float(ga.abs().max()) == 0.0) == zero
    for x, y in zip(a + [sa], b + [sb]):
        assert torch.equal(x, y), (n, zero, wd)
    assert not torch.equal(a[0], p) and float(a[1].abs().max()) > 0 and float(a[2].abs().max()) > 0
    assert torch.equal(sb, b[0].to(torch.bfloat16)) and torch.equal(sa, a[0].to(torch.bfloat16))


def test_adam_whole_bucket_equals_a_live_table_covering_it():
    """The Adam rule with no live table (what parallel.FlatAdam launches) against the same rule with the one live range [0, n): the
    same arithmetic in the same kernel, so every buffer is bit-identical after three steps; and the snapshot is the bf16 cast of the
    updated weights.  The float4 form and the scalar form (n = 65539), both ZERO forms, weight_decay 0 and 0.01."""
    for n in (1 << 16, (1 << 16) + 3):
        for zero in (False, True):
            for wd in (0.0, 0.01):
                _whole_bucket_against_full_table(n, zero, wd)


# ------------------------------------------------------------------------------------------------ against torch on the golden model
@pytest.mark.parametrize("rule,lr,wd,clip", CASES, ids=RULES)
def test_every_rule_tracks_torch_on_the_golden_model(golden, rule, lr, wd, clip):
    g = golden("subgc_train")
    w = g.group("weights")
    batch = g.tensors("inputs")
    o = ns(rule, lr, wd)
    m = build(g, w, True)
    fopt = optim.build_optimizer(m, o, clip_norm=clip)
    ref = TorchSide(g, w, o, clip)
    skipped = optim.skipped_param_names(m)
    before = {k: m.P(k).detach().clone() for k in skipped}
    for it in range(8):
        loss = fused_step(m, fopt, batch)
        rl = ref.step(batch)
        close(loss, rl, f"{rule}: loss at step {it}", atol=2e-4, rtol=1e-4)
    compare_params(m, ref.orc, rule, rule)
    if clip < 8.0:
        assert max(ref.norms) > clip, "the clip should have been active"
    if rule == "sgd":                       # weight decay 5e-4 on every step: a skipped parameter would have moved
        assert len(skipped) == 19
        for k in skipped:
            assert torch.equal(m.P(k).detach(), before[k]), k
    sd = fopt.state_dict()
    tsd = ref.opt.state_dict()
    assert sorted(sd["state"]) == sorted(tsd["state"])
    for i, e in tsd["state"].items():
        assert sorted(sd["state"][i]) == sorted(e)
        for k, v in e.items():
            close(sd["state"][i][k], v, f"{rule}: state {i} {k}", atol=1e-5, rtol=1e-3)


def test_warmup_schedule_through_param_groups(golden):
    """train.py:107-124: lr = iteration * learning_rate / warmup_n for iteration <= warmup_n, then the (un-decayed) rate, written into
    every param group (misc/utils.py:158-160) before each step."""
    g = golden("subgc_train")
    w = g.group("weights")
    batch = g.tensors("inputs")
    o = ns("adam", 1e-3, 0.0)
    m = build(g, w, True)
    fopt = optim.build_optimizer(m, o)
    ref = TorchSide(g, w, o, 10.0)
    warmup_n = 4
    for it in range(8):
        cur = it * o.learning_rate / warmup_n if it <= warmup_n else o.learning_rate
        for opt_ in (fopt, ref.opt):
            for group in opt_.param_groups:
                group["lr"] = cur
        if it == 0:                                                    # lr 0: the state moves, the weights do not
            w0 = m.flat_params.clone()
        close(fused_step(m, fopt, batch), ref.step(batch), f"loss at {it}", atol=2e-4, rtol=1e-4)
        if it == 0:
            assert torch.equal(m.flat_params, w0) and fopt.t == 1
    compare_params(m, ref.orc, "warm-up", "adam")


# ------------------------------------------------------------------------------------------------ resume
def _save(obj):
    buf = io.BytesIO()
    torch.save(obj, buf)
    buf.seek(0)
    return torch.load(buf)


@pytest.mark.parametrize("rule,lr,wd,clip", CASES, ids=RULES)
def test_resume_fused_to_fused_is_bit_identical(golden, rule, lr, wd, clip):
    g = golden("subgc_train")
    w = g.group("weights")
    batch = g.tensors("inputs")
    o = ns(rule, lr, wd)
    with ops.deterministic():
        m = build(g, w, True, drop_prob_lm=0.0)
        fopt = optim.build_optimizer(m, o, clip_norm=clip)
        straight = [fused_step(m, fopt, batch) for _ in range(8)]
        a = build(g, w, True, drop_prob_lm=0.0)
        aopt = optim.build_optimizer(a, o, clip_norm=clip)
        first = [fused_step(a, aopt, batch) for _ in range(4)]
        ckpt = _save({"model": a.state_dict(), "optimizer": aopt.state_dict()})
        del a, aopt
        b = build(g, {k: v for k, v in ckpt["model"].items()}, True, drop_prob_lm=0.0)
        bopt = optim.build_optimizer(b, ns(rule, 123.0, wd), clip_norm=clip)          # the rate comes from the file
        bopt.load_state_dict(ckpt["optimizer"])
        assert bopt.param_groups[0]["lr"] == lr
        second = [fused_step(b, bopt, batch) for _ in range(4)]
        torch.cuda.synchronize()
    assert first + second == straight
    assert torch.equal(b.flat_params, m.flat_params), rule
    sb, sm = bopt.state_dict(), fopt.state_dict()
    for i, e in sm["state"].items():
        for k, v in e.items():
            assert torch.equal(sb["state"][i][k], v), (rule, i, k)


@pytest.mark.parametrize("rule,lr,wd,clip", CASES, ids=RULES)
def test_resume_between_torch_and_fused(golden, rule, lr, wd, clip):
    """torch (the reference's optimizer) 4 steps -> optimizer.pth -> fused 4 steps, and fused 4 -> torch 4: both continue the
    uninterrupted torch trajectory."""
    g = golden("subgc_train")
    w = g.group("weights")
    batch = g.tensors("inputs")
    o = ns(rule, lr, wd)
    ref = TorchSide(g, w, o, clip)
    for _ in range(8):
        ref.step(batch)
    # torch -> fused
    t4 = TorchSide(g, w, o, clip)
    for _ in range(4):
        t4.step(batch)
    ckpt = _save({"model": {k: p.detach().clone() for k, p in t4.orc.P.items()}, "optimizer": t4.opt.state_dict()})
    m = build(g, ckpt["model"], True)
    fopt = optim.build_optimizer(m, o, clip_norm=clip)
    fopt.load_state_dict(ckpt["optimizer"])
    for _ in range(4):
        fused_step(m, fopt, batch)
    compare_params(m, ref.orc, f"{rule} torch -> fused", rule)
    # fused -> torch
    m = build(g, w, True)
    fopt = optim.build_optimizer(m, o, clip_norm=clip)
    for _ in range(4):
        fused_step(m, fopt, batch)
    ckpt = _save({"model": weights_of(m), "optimizer": fopt.state_dict()})
    t = TorchSide(g, {k: ckpt["model"][k] for k in w}, o, clip)          # the reference's module tree registers in ITS order
    t.opt.load_state_dict(ckpt["optimizer"])
    for _ in range(4):
        t.step(batch)
    for k, p in t.orc.P.items():
        if not (k == NOISE_ONLY and rule in ADAPTIVE):
            close(p, ref.orc.P[k], f"{rule} fused -> torch: param {k}", atol=PATOL, rtol=PRTOL)


# ------------------------------------------------------------------------------------------------ plumbing
def test_bf16_snapshot_and_decode_follow_the_step(golden):
    g = golden("subgc_greedy")
    w = golden("subgc_train").group("weights")
    m = build(g, w, True, compute_dtype="bf16")
    fopt = optim.build_optimizer(m, ns("adamw", 5e-2, 0.0))
    b = {k: v.to(DEV) for k, v in g.tensors("inputs").items()}
    sopt = dict(g.meta["sample_opt"], sample_max=1, beam_size=1)
    m.eval()
    first = m(*synthetic.sample_args(b), opt=sopt, mode="sample")
    grads = m.flatten_grads()
    grads.copy_(torch.randn(grads.numel(), generator=torch.Generator().manual_seed(5)).to(DEV))
    fopt.step()
    snap = m.weights_b16()
    assert torch.equal(snap, m.flat_params.to(torch.bfloat16))
    again = m(*synthetic.sample_args(b), opt=sopt, mode="sample")
    fresh = build(g, weights_of(m), False, compute_dtype="bf16")(*synthetic.sample_args(b), opt=sopt, mode="sample")
    assert torch.equal(again[0], fresh[0])
    torch.testing.assert_close(again[1], fresh[1], atol=1e-5, rtol=1e-5)
    assert not torch.allclose(first[1], again[1])


def test_grad_bucket_reducer_at_world_size_one(golden):
    """GradBucketReducer(optimizer=...) drives begin_step / accumulate; at world size 1 the step equals the one without a reducer."""
    g = golden("subgc_train")
    w = g.group("weights")
    batch = g.tensors("inputs")
    runs = []
    for use in (False, True):
        m = build(g, w, True)
        fopt = optim.build_optimizer(m, ns("sgdm", 5e-2, 1e-3), clip_norm=2.0)
        red = parallel.GradBucketReducer(m, optimizer=fopt) if use else None
        assert red is None or fopt.reducer is red
        for _ in range(3):
            if red is None:
                fused_step(m, fopt, batch)
                continue
            red.prepare()
            b = {k: v.to(DEV) for k, v in batch.items()}
            out = models.LossWrapper(m, None)(b["fc_feats"], b["att_feats"], b["labels"], b["masks"], b["att_masks"], None, None, None,
                                              b["obj_dist"], None, b["rel_ind"], None, b["pred_dist"], b["gpn_obj_ind"], b["gpn_pred_ind"],
                                              b["gpn_nrel_ind"], b["gpn_pool_mtx"])
            (out["lang_loss"] + out["gpn_loss"]).backward()
            red.finish(average=False)
            fopt.step(grad_scale=1.0)
        if red is not None:
            red.close()
        runs.append(m.flat_params.clone())
    close(runs[0], runs[1], "reducer vs none", atol=1e-6, rtol=1e-6)


def test_zero_fold_makes_zero_grad_free_and_step_refuses_stale_gradients(golden, monkeypatch):
    g = golden("subgc_train")
    m = build(g, g.group("weights"), True)
    fopt = optim.build_optimizer(m, ns("rmsprop", 1e-3, 0.0), fold_zero_grad=True)
    fused_step(m, fopt, g.tensors("inputs"))
    assert m.__dict__.get("_grads_are_zero") is not None
    views = m.__dict__["_grad_views"]
    fills = []
    real = ops.fill_
    monkeypatch.setattr(ops, "fill_", lambda x, v: fills.append(x.numel()) or real(x, v))
    fopt.zero_grad()
    assert fills == [] and m.__dict__["_grad_views"] is views
    assert float(m.flat_grads.abs().max()) == 0.0
    assert all(p.grad is views[n] for n, p in m.named_parameters())
    monkeypatch.setattr(ops, "fill_", real)
    # a .grad that is not a view of the bucket: this step's gradients would not be in it
    p = m.P("logit.weight")
    p.grad = None
    with pytest.raises(RuntimeError, match="not a view"):
        fopt.step()
    p.grad = torch.zeros_like(p)
    with pytest.raises(RuntimeError, match="not a view"):
        fopt.step()
    fopt.zero_grad()
    fopt.step()                                                        # bound again: fine


HARMLESS = ("view", "reshape", "empty", "as_strided", "detach", "alias", "slice", "select", "t.default", "_unsafe_view", "lift_fresh",
            "set_", "resize_", "stride", "sym_", "_local_scalar_dense")


class Watch(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.seen = collections.Counter()

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        r = func(*args, **(kwargs or {}))
        name = str(func)
        if not any(h in name for h in HARMLESS):
            ts = [t for t in (list(args) + ([r] if torch.is_tensor(r) else [])) if torch.is_tensor(t)]
            if any(t.is_cuda for t in ts):
                self.seen[name] += 1
        return r


@pytest.mark.parametrize("rule", ["adamw", "sgdmom", "adagrad"])
def test_fused_step_issues_no_aten_device_kernel(golden, rule):
    g = golden("subgc_train")
    m = build(g, g.group("weights"), True, compute_dtype="bf16")
    fopt = optim.build_optimizer(m, ns(rule, 1e-3, 1e-3))
    fused_step(m, fopt, g.tensors("inputs"))
    fopt.zero_grad()
    m.flat_grads.normal_()
    with Watch() as wt:
        fopt.step()
        fopt.step(zero_grad=True)
        fopt.zero_grad()
    assert not wt.seen, dict(wt.seen)
