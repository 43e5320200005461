"""The label-smoothed language loss (`--label_smoothing`, misc/utils.py:126-156) on the device: the four entry points of
include/subgc_criterion_hip.h, the stand-alone criterion, and the three model paths (unpacked DecoderFn, packed loss-only decoder, bf16
storage) against the fixtures the reference's own LabelSmoothing wrote and the fp64 closed form that test_label_smoothing_cpu.py ties to
them.  Tolerances: DESIGN 4.M (label_smoothing_golden.loss_bound) for the kernels; the project's fp32 parity tolerances (lang_loss 1e-4,
gradients atol 2e-4 / rtol 2e-3) and SURVEY 8(c)'s bf16 tolerance (loss atol 5e-2, gradients by direction and norm as in
test_bf16_storage_gpu.py) for the model."""
import argparse
import collections
import os

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import label_smoothing_golden as G
import bench
from subgc import ops, parallel, synthetic
from subgc._lib import SubgcError
import subgc.models as models

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = G.U
SMOOTH = argparse.Namespace(label_smoothing=0.1)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def seeded(rows, V, offset, seed):
    """rows x V logits randn * 3 + offset (fp32), targets that include 0 and V - 1, a mask with one zero."""
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, V, generator=gen) * 3.0 + offset).float()
    tgt = torch.randint(0, V, (rows,), generator=gen)
    tgt[0], tgt[1] = 0, V - 1
    msk = torch.ones(rows)
    msk[2] = 0.0
    return x, tgt.view(rows, 1), msk.view(rows, 1)


# ----------------------------------------------------------------------------------------------------------------- 1. the fixture
def test_standalone_criterion_matches_the_reference_fixture():
    meta, arr = G.load_case()
    target, mask = dev(arr["target"]), dev(arr["mask"])                       # wider than T: the criterion truncates them
    for s, key in zip(meta["smoothings"], meta["keys"]):
        logp = dev(arr["logp"]).requires_grad_(True)
        loss = models.LabelSmoothing(smoothing=s)(logp, target, mask)
        loss.backward()
        tol = 2 * G.loss_bound(arr["logp"], arr["target"], arr["mask"], s) + 8 * U * abs(float(arr["loss_" + key]))      # both sides are fp32
        print(f"s={s}: loss {float(loss.detach()):.8f} ref {float(arr['loss_' + key]):.8f} tol {tol:.2e}")
        assert abs(float(loss) - float(arr["loss_" + key])) <= tol, s
        np.testing.assert_allclose(logp.grad.cpu().numpy(), arr["dlogp_" + key], rtol=8 * U, atol=0, err_msg=str(s))


# ----------------------------------------------------------------------------------------------- 2. fp64 closed form, seeded inputs
@pytest.mark.parametrize("offset", [50.0, -20.0])
@pytest.mark.parametrize("V", [37, 256, 1001, 3000, 9488, 10300])
def test_criterion_matches_the_fp64_closed_form(V, offset):
    """7 rows; V covers the scalar and the 4-column forms, fewer columns than lanes and every PER bucket (4; 16 at V = 3000; 40; 64).  (a) the
    stand-alone criterion on fp32 log-probabilities, (b) the raw-logit form (row_lse_sum + lse) the packed decoder uses, where the shared
    offset of the logits must not cost digits."""
    rows, s = 7, 0.1
    x, tgt, msk = seeded(rows, V, offset, 100 + V)
    lp64 = G.log_softmax64(x.numpy())
    # (a) log-probabilities rounded to fp32 ARE the input: the reference is the closed form of those numbers
    lp32 = lp64.astype(np.float32)
    want, dwant = G.closed_form(lp32.reshape(rows, 1, V), tgt.numpy(), msk.numpy(), s)
    logp = dev(lp32.reshape(rows, 1, V)).requires_grad_(True)
    loss = models.LabelSmoothing(smoothing=s)(logp, tgt.to(DEV), msk.to(DEV))
    loss.backward()
    tol = G.loss_bound(lp32.reshape(rows, 1, V), tgt.numpy(), msk.numpy(), s)
    print(f"V={V} offset={offset}: logp form |d| {abs(float(loss) - want):.3e} tol {tol:.3e} loss {want:.6f}")
    assert abs(float(loss) - want) <= tol
    np.testing.assert_allclose(logp.grad.cpu().numpy(), dwant, rtol=8 * U, atol=0)
    # (b) raw logits: the reference is the closed form of the fp64 log-softmax of the same fp32 logits
    want, _ = G.closed_form(lp64.reshape(rows, 1, V), tgt.numpy(), msk.numpy(), s)
    xd = x.to(DEV)
    lse, slp = ops.row_lse_sum(xd)
    loss_raw, scratch = ops.smoothed_nll_fwd(xd.view(rows, 1, V), tgt.to(DEV), msk.to(DEV), slp, s, lse=lse)
    lse64 = x.double().logsumexp(1).numpy()
    tol = G.loss_bound(lp64.reshape(rows, 1, V), tgt.numpy(), msk.numpy(), s, lse=lse64)
    print(f"V={V} offset={offset}: raw form  |d| {abs(float(loss_raw) - want):.3e} tol {tol:.3e}")
    assert abs(float(loss_raw) - want) <= tol
    assert torch.equal(lse, ops.row_lse(xd))                                  # the same lse as the existing row pass, bit for bit
    per = -(-V // 256)                                                        # slp: the sum's own error + V times the error of one x - lse
    slp_tol = (per + 10) * U * np.abs(lp64).sum(1).max() + V * U * (3 * np.abs(lse64).max() + per + 12 + np.abs(lp64).max())
    assert np.abs(slp.cpu().numpy() - lp64.sum(1)).max() <= slp_tol
    assert float(scratch[1]) == float(msk.sum())


# --------------------------------------------------------------------------------------------------------- 3. kernel-form agreement
@pytest.mark.parametrize("V,pad", [(37, 0), (256, 0), (256, 1), (256, 4), (1001, 3)])
def test_fused_backward_equals_the_two_step_backward(V, pad):
    """subgc_smoothed_logsoftmax_bwd against subgc_smoothed_nll_bwd followed by the existing subgc_log_softmax_rows_bwd, on
    log-probabilities and on raw logits + lse, fp32 and bf16 output, with inactive and masked rows, aligned (pad 0 / 4 at V % 4 == 0: four
    columns per lane) and unaligned output rows (one column per lane).  The two-step form sums d(logp) over the row in fp32
    (ceil(V / 256) terms per lane + the tree): |difference| <= |g| (ceil(V / 256) + 16) u, since softmax and true_dist are <= 1."""
    S, T, s = 2, 4, 0.1
    rows = S * T
    x, tgt, msk = seeded(rows, V, 5.0, 7 + V)
    tgt, msk = tgt.view(S, T).to(DEV), msk.view(S, T).to(DEV)
    active = torch.ones(rows, dtype=torch.int32); active[5] = 0
    active = active.to(DEV)
    xd = x.to(DEV)
    logp = ops.log_softmax_rows_(xd.clone(), active)                          # row 5 is a zero row, row 2 is masked
    _, slp = ops.row_lse_sum(logp, raw=False)
    loss, scratch = ops.smoothed_nll_fwd(logp.view(S, T, V), tgt, msk, slp, s)
    dloss = torch.full((), 0.7, device=DEV)
    g = 0.7 / float(scratch[1])
    tol = g * (-(-V // 256) + 16) * U
    dlogp = ops.smoothed_nll_bwd(tgt, msk, scratch, dloss, s, S, T, V)
    two = ops.log_softmax_rows_bwd(logp, dlogp.view(rows, V), torch.empty(rows, V, device=DEV), active)
    new = lambda dt: torch.full((rows, V + pad), 7.0, device=DEV, dtype=dt)[:, :V]      # the kernel must write every element of its rows
    fused = ops.smoothed_logsoftmax_bwd(logp, tgt, msk, scratch, dloss, s, new(torch.float32), active, S, T, V)
    err = float((fused - two).abs().max())
    print(f"V={V} pad={pad}: fused vs two-step {err:.3e} tol {tol:.3e}")
    assert err <= tol
    assert not fused[2].any() and not fused[5].any() and not two[2].any() and fused[0].any()      # masked / inactive rows: exactly zero
    # raw logits + lse: the same gradient on the rows that are live (a raw row has no `active` zeroing of its own)
    lse, slp_raw = ops.row_lse_sum(xd)
    fused_raw = ops.smoothed_logsoftmax_bwd(xd, tgt, msk, scratch, dloss, s, new(torch.float32), active, S, T, V, lse=lse)
    assert float((fused_raw - fused).abs().max()) <= g * 4 * U * (1 + float(lse.abs().max()))      # exp(x - lse) against exp(lp): ulp(lse) in the exponent
    assert not fused_raw[2].any() and not fused_raw[5].any()
    # bf16 output = the fp32 output rounded once (same arithmetic, round-to-nearest-even at the store)
    for src, kw in ((logp, {}), (xd, {"lse": lse})):
        want = ops.smoothed_logsoftmax_bwd(src, tgt, msk, scratch, dloss, s, new(torch.float32), active, S, T, V, **kw)
        got = ops.smoothed_logsoftmax_bwd(src, tgt, msk, scratch, dloss, s, new(torch.bfloat16), active, S, T, V, **kw)
        assert torch.equal(got.float().cpu(), want.cpu().to(torch.bfloat16).float())
    # the forward's two forms: raw logits + lse against log-probabilities (inactive rows aside: all rows active here)
    all_on = torch.ones(rows, dtype=torch.int32, device=DEV)
    lp_all = ops.log_softmax_rows_(xd.clone(), all_on)
    _, slp_lp = ops.row_lse_sum(lp_all, raw=False)
    l_lp, _ = ops.smoothed_nll_fwd(lp_all.view(S, T, V), tgt, msk, slp_lp, s)
    l_raw, _ = ops.smoothed_nll_fwd(xd.view(S, T, V), tgt, msk, slp_raw, s, lse=lse)
    lp64 = G.log_softmax64(x.numpy()).reshape(S, T, V)
    bound = G.loss_bound(lp64, tgt.cpu().numpy(), msk.cpu().numpy(), s, lse=lse.cpu().numpy().astype(np.float64))
    assert abs(float(l_lp) - float(l_raw)) <= 2 * bound


# ---------------------------------------------------------------------------------------------------- 4. forward-only properties
def test_den_override_accounts_for_the_zero_rows_a_prefix_call_does_not_see():
    """The packed decoder's call: only the rows before the early break are given, with the denominator of ALL mask entries.  That must be
    the loss of the full call in which the remaining rows are zero rows, one of them masked in (it adds m * H) and the others masked out."""
    V, s, n_all, n_seen = 300, 0.1, 12, 8
    x, tgt, msk = seeded(n_all, V, 0.0, 3)
    msk[n_seen:] = 0.0
    msk[n_seen + 1] = 1.0                                                      # a masked-in row after the break
    lp = torch.log_softmax(x, 1)
    lp[n_seen:] = 0.0
    lp, tgt, msk = lp.to(DEV), tgt.to(DEV), msk.to(DEV)
    _, slp = ops.row_lse_sum(lp, raw=False)
    full, sc_full = ops.smoothed_nll_fwd(lp.view(n_all, 1, V), tgt, msk, slp, s)
    den = msk.sum().view(1)
    part, sc_part = ops.smoothed_nll_fwd(lp[:n_seen].view(n_seen, 1, V), tgt[:n_seen], msk[:n_seen], slp[:n_seen].contiguous(), s, den=den)
    want, _ = G.closed_form(lp.cpu().numpy().reshape(n_all, 1, V), tgt.cpu().numpy(), msk.cpu().numpy(), s)
    tol = G.loss_bound(lp.cpu().numpy().reshape(n_all, 1, V), tgt.cpu().numpy(), msk.cpu().numpy(), s)
    print(f"full {float(full):.8f} prefix + den_override {float(part):.8f} fp64 {want:.8f} tol {tol:.2e}")
    assert abs(float(full) - want) <= tol and abs(float(part) - want) <= tol
    assert float(sc_part[1]) == float(sc_full[1]) == float(den)
    conf, e, H = G.constants(s, V)
    no_rule, _ = ops.smoothed_nll_fwd(lp[:n_seen].view(n_seen, 1, V), tgt[:n_seen], msk[:n_seen], slp[:n_seen].contiguous(), s)
    assert abs(float(no_rule) * float(msk[:n_seen].sum()) + H - want * float(den)) < 1e-4      # the term is H per unseen masked-in row
    # under NLL (smoothing 0) the same rows add nothing: H = 0
    z_full, _ = ops.smoothed_nll_fwd(lp.view(n_all, 1, V), tgt, msk, slp, 0.0)
    z_part, _ = ops.smoothed_nll_fwd(lp[:n_seen].view(n_seen, 1, V), tgt[:n_seen], msk[:n_seen], slp[:n_seen].contiguous(), 0.0, den=den)
    nll, _ = ops.masked_nll_fwd(lp.view(n_all, 1, V), tgt, msk)
    assert abs(float(z_full) - float(nll)) <= 8 * U * abs(float(nll)) and abs(float(z_part) - float(nll)) <= 8 * U * abs(float(nll))


def test_equal_inputs_give_equal_bits_with_the_deterministic_mode_off_and_on():
    S, T, V, s = 3, 5, 9488, 0.1
    x, tgt, msk = seeded(S * T, V, 2.0, 11)
    xd, tgt, msk = x.to(DEV), tgt.view(S, T).to(DEV), msk.view(S, T).to(DEV)
    dloss = torch.ones((), device=DEV)

    def run():
        lse, slp = ops.row_lse_sum(xd)
        loss, sc = ops.smoothed_nll_fwd(xd.view(S, T, V), tgt, msk, slp, s, lse=lse)
        d = ops.smoothed_logsoftmax_bwd(xd, tgt, msk, sc, dloss, s, torch.empty(S * T, V, device=DEV), None, S, T, V, lse=lse)
        return lse, slp, loss, sc, d, ops.smoothed_nll_bwd(tgt, msk, sc, dloss, s, S, T, V)

    a, b = run(), run()
    with ops.deterministic():
        c = run()
    for p, q, r in zip(a, b, c):
        assert torch.equal(p, q) and torch.equal(p, r)


def test_debug_bounds_refuses_a_target_equal_to_V():
    S, T, V = 2, 3, 20
    x, tgt, msk = seeded(S * T, V, 0.0, 5)
    lp = torch.log_softmax(x, 1).to(DEV)
    tgt = tgt.view(S, T).clone()
    tgt[1, 1] = V
    tgt, msk = tgt.to(DEV), msk.view(S, T).to(DEV)
    _, slp = ops.row_lse_sum(lp, raw=False)
    with ops.debug_bounds():
        with pytest.raises(SubgcError, match=r"smoothed_nll_fwd: target \(word ids\)"):
            ops.smoothed_nll_fwd(lp.view(S, T, V), tgt, msk, slp, 0.1)
    loss, _ = ops.smoothed_nll_fwd(lp.view(S, T, V), tgt, msk, slp, 0.1)          # mode off: clamped like the NLL kernels clamp it
    assert torch.isfinite(loss)
    with pytest.raises(SubgcError, match="smoothing 1.5 is outside"):
        ops.smoothed_nll_fwd(lp.view(S, T, V), tgt, msk, slp, 1.5)


# ------------------------------------------------------------------------------------------------------------------- model level
def build(g, weights, **over):
    m = models.setup(g.opt(caption_model="topdown", gpn_drop_prob=0.0, **over))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    return m.to(DEV).train()


def run_train(m, batch, opt, packed=None):
    if packed is not None:
        m.packed_decoder = packed
    lw = models.LossWrapper(m, opt)
    b = {k: v.to(DEV) for k, v in batch.items()}
    m.flatten_grads()
    out = lw(*bench.lw_args(b))
    if packed is not None:                                                      # the path asked for is the path that ran
        assert ("Packed" in type(out["lang_loss"].grad_fn).__name__) == bool(packed), type(out["lang_loss"].grad_fn).__name__
    models.total_loss(out).backward()
    torch.cuda.synchronize()
    return out


def close(a, b, name, atol, rtol):
    a = a.detach().float().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    np.testing.assert_allclose(a, np.asarray(b), atol=atol, rtol=rtol, err_msg=name)


@pytest.mark.parametrize("packed", [True, False])
def test_model_matches_the_reference_trained_with_label_smoothing(golden, packed):
    """The reference model with LabelSmoothing(smoothing=0.1) as its language criterion (label_smoothing_train.npz): lang_loss within 1e-4,
    every live gradient within atol 2e-4 / rtol 2e-3, the project's fp32 parity tolerances, through both decoder Functions."""
    g, ref = golden("subgc_train"), G.load_train()
    m = build(g, g.group("weights"))
    out = run_train(m, g.tensors("inputs"), SMOOTH, packed)
    print(f"packed={packed}: lang_loss {float(out['lang_loss']):.7f} ref {float(ref['lang_loss']):.7f}")
    close(out["lang_loss"], ref["lang_loss"], "lang_loss", atol=1e-4, rtol=1e-4)
    close(out["gpn_loss"], ref["gpn_loss"], "gpn_loss", atol=1e-4, rtol=1e-4)
    dead = set(g.meta["dead_params"])
    for k, p in m.named_parameters():
        if k in dead:
            assert float(p.grad.abs().max()) == 0.0, k
        else:
            close(p.grad, ref[k], "grad " + k, atol=2e-4, rtol=2e-3)
    plain = golden("subgc_train").group("out")
    assert abs(float(out["lang_loss"]) - float(plain["lang_loss"])) > 0.1       # not the NLL


def early_break_batch(batch):
    """Captions of at most 6 words: labels[:, t] is all zero from t = 7 on (the reference's loop breaks there), masks of len + 2 ones
    as the loader builds them -- and ONE mask entry beyond the break, so a masked-in zero row exists."""
    b = {k: v.clone() for k, v in batch.items()}
    gen = torch.Generator().manual_seed(11)
    S = b["labels"].size(0)
    b["labels"].zero_(); b["masks"].zero_()
    for j in range(S):
        n = 1 + (j * 5) % 6
        b["labels"][j, 1:n + 1] = torch.randint(1, 51, (n,), generator=gen)
        b["masks"][j, :n + 2] = 1
    b["masks"][1, 12] = 1
    assert not b["labels"][:, 7:].any() and b["labels"][:, 6].any() and b["labels"].size(1) > 13
    return b


@pytest.mark.parametrize("ss_prob", [0.0, 0.25])
def test_packed_equals_unpacked_with_a_masked_in_row_after_the_early_break(golden, ss_prob):
    """Dropout 0, smoothing 0.1, golden-size model.  The packed decoder never sees the rows after the break and owes the numerator m * H
    for the masked-in one; the unpacked decoder has it as a zero row.  Loss and gradients as tests/test_packed_gpu.py requires of the
    two paths; the loss also against the fp64 closed form of the unpacked path's own log-probabilities (zero rows included)."""
    g = golden("subgc_train")
    m = build(g, g.group("weights"), sampling_prob=ss_prob)
    assert m.ss_prob == ss_prob
    batch = early_break_batch(g.tensors("inputs"))
    S, T = batch["labels"].size(0), batch["labels"].size(1) - 1
    gen = torch.Generator().manual_seed(77)
    inj = (torch.rand(T, S, generator=gen).to(DEV), torch.rand(T, S, generator=gen).to(DEV))
    res = {}
    for packed in (False, True):
        m.injected_ss = inj if ss_prob > 0 else None
        out = run_train(m, batch, SMOOTH, packed)
        res[packed] = (float(out["lang_loss"]), m.flat_grads.clone())
    (l0, g0), (l1, g1) = res[False], res[True]
    print(f"ss={ss_prob}: unpacked {l0:.8f} packed {l1:.8f}")
    assert abs(l0 - l1) < 2e-5 * max(1.0, abs(l0))
    scale = float(g0.abs().max())
    np.testing.assert_allclose(g1.cpu().numpy(), g0.cpu().numpy(), atol=2e-5 * scale + 1e-7, rtol=2e-4)
    if ss_prob == 0:
        with torch.no_grad():
            outputs, _, _ = m(*synthetic.forward_args({k: v.to(DEV) for k, v in batch.items()}))
        lp = outputs.cpu().numpy()
        assert not lp[:, 7:].any() and lp[:, 6].any()                           # the rows after the break are zero rows
        want, _ = G.closed_form(lp, batch["labels"][:, 1:].numpy(), batch["masks"][:, 1:].numpy(), 0.1)
        conf, e, H = G.constants(0.1, lp.shape[2])
        assert abs(l0 - want) < 1e-4 and abs(l1 - want) < 1e-4
        # the masked-in zero row is worth H / den: leaving it out of the packed numerator would miss by that much
        assert abs(H) / float(batch["masks"][:, 1:].sum()) > 1e-2


@pytest.mark.parametrize("packed", [True, False])
def test_bf16_storage_path_follows_the_fp32_path(golden, packed):
    """compute_dtype = bf16 (d(logits) written bf16 by the fused backward) against the fp32 HIP path on the same weights and batch, at
    SURVEY 8(c)'s bf16 tolerance as tests/test_bf16_storage_gpu.py applies it to this golden case: loss atol 5e-2; gradients by direction
    (cosine > 0.995 for the decoder's large tensors, > 0.95 for every live one) and norm (10 %)."""
    g = golden("subgc_train")
    cos = lambda a, b: float((a.double().flatten() @ b.double().flatten()) / (a.double().norm() * b.double().norm() + 1e-30))
    ref_m = build(g, g.group("weights"))
    ref = run_train(ref_m, g.tensors("inputs"), SMOOTH, packed)
    m = build(g, g.group("weights"), compute_dtype="bf16")
    assert m.bf16_storage
    out = run_train(m, g.tensors("inputs"), SMOOTH, packed)
    print(f"packed={packed}: bf16 {float(out['lang_loss']):.6f} fp32 {float(ref['lang_loss']):.6f}")
    assert abs(float(out["lang_loss"]) - float(ref["lang_loss"])) <= 5e-2
    assert float(out["lang_loss"]) != float(ref["lang_loss"])                   # bf16 arithmetic really ran
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


@pytest.mark.parametrize("packed", [True, False])
def test_smoothing_off_is_bit_identical_to_the_plain_criterion(golden, packed):
    """label_smoothing = 0 through LossWrapper: the launches of LanguageModelCriterion, hence its bits (deterministic mode: the step has
    float atomics otherwise).  Holds before this option existed as well: an `opt` attribute nobody reads."""
    g = golden("subgc_train")
    m = build(g, g.group("weights"))
    res = []
    with ops.deterministic():
        for opt in (None, argparse.Namespace(label_smoothing=0), argparse.Namespace(label_smoothing=0.0)):
            out = run_train(m, g.tensors("inputs"), opt, packed)
            res.append((out["lang_loss"].clone(), m.flat_grads.clone()))
    for loss, grads in res[1:]:
        assert torch.equal(loss, res[0][0]) and torch.equal(grads, res[0][1])
    close(res[0][0], golden("subgc_train").group("out")["lang_loss"], "lang_loss", atol=1e-4, rtol=1e-4)


# ops that only make views / allocate / move the plan counts to pinned memory (the list of tests/test_no_aten_gpu.py)
HARMLESS = ("view", "reshape", "empty", "as_strided", "detach", "alias", "slice", "select", "transpose", "permute", "expand", "unsqueeze",
            "squeeze", "_unsafe_view", "t.default", "unbind", "split", "narrow", "pin_memory", "is_pinned", "record_stream", "_reshape_alias",
            "lift_fresh", "unfold", "chunk", "set_", "resize_", "stride", "sym_", "is_same_size", "_local_scalar_dense")


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
                host_copy = ("copy_" in name or "_to_copy" in name) and any(not t.is_cuda for t in ts)   # host <-> device: a DMA, not a kernel
                if not host_copy:
                    self.seen[name] += 1
        return r


@pytest.mark.skipif(os.getenv("SUBGC_POISON_EMPTY") == "1", reason="the poisoned run fills every torch.empty buffer with an ATen fill_ by design")
def test_smoothed_packed_step_issues_no_aten_device_kernel():
    """The method of tests/test_no_aten_gpu.py on the smoothed step (forward, backward, fused clip + Adam) through the packed decoder."""
    torch.manual_seed(3)
    m = models.setup(argparse.Namespace(**bench.KAR)).to(DEV).train()
    assert m.packed_decoder
    lw = models.LossWrapper(m, SMOOTH)
    b = {k: v.to(DEV) for k, v in synthetic.make_train_batch(8, seed=5).items()}
    adam = parallel.FlatAdam(m)
    one = torch.ones((), device=DEV)

    def step():
        m.flatten_grads()
        out = lw(*bench.lw_args(b))
        models.total_loss(out).backward(one)
        adam.step()
        return out

    step()
    step()
    torch.cuda.synchronize()
    with Watch() as w:
        out = step()
    torch.cuda.synchronize()
    assert not w.seen, dict(w.seen)
    assert out["lang_loss"] is m.fused_lang_loss and out["lang_loss"].grad_fn is not None and "Packed" in type(out["lang_loss"].grad_fn).__name__
