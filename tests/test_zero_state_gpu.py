"""ops.ZERO_STATE_SKIP: step 0 of the train decoder forms no product against the zero initial state (forward: plain attention-LSTM cell,
language-LSTM product over K = 2R; backward: no gradient of the initial state) and the weight gradients against a previous state skip
the rows of step 0.  The switch only removes terms that are exact zeros, so the train step with it equals the train step without it up
to the order of the remaining sums: the tolerances are the project's own for a reordered sum (fp32: test_packed_gpu's packed ==
unpacked bound, bf16: test_poison_gpu's bound)."""
import argparse
import functools

import numpy as np
import pytest
import torch

from subgc import ops, synthetic
import subgc.functions as F_
import subgc.models as models
from test_packed_gpu import DEV, OPT

pytestmark = pytest.mark.gpu

BIASES = ("core.att_lstm.bias_ih", "core.att_lstm.bias_hh", "core.lang_lstm.bias_ih", "core.lang_lstm.bias_hh")


def _opt(kind, ss):
    opt = dict(OPT, sampling_prob=ss)
    if kind.startswith("fullgc"):
        opt.update(use_gpn=0, noun_fuse=0, pred_emb_type=2, gcn_layers=4, gcn_residual=1, gcn_bn=1)
    if "bf16" in kind:
        opt.update(compute_dtype="bf16")
    if "dropout" in kind:
        opt.update(drop_prob_lm=0.5)
    return opt


def _batch(which):
    mk = lambda **k: synthetic.make_train_batch(6, D=256, vocab=300, n_obj_cls=60, seed=9, fc_size=256, **k)
    if which == "ragged":
        return mk(min_len=2, max_len=16)
    if which == "no_words":                 # every sentence is dead after step 0: the first step is the last, the cut weight gradients have K = 0
        b = mk(min_len=1, max_len=16)
        b["labels"][:] = 0
        b["masks"][:, 2:] = 0
        return b
    if which == "two_empty":                # two sentences without words among longer ones: M[1] < M[0]
        b = mk(min_len=1, max_len=16)
        b["labels"][3:5] = 0
        b["masks"][3:5, 2:] = 0
        return b
    assert which == "equal_len"             # no row ever dies
    return mk(min_len=7, max_len=7)


@functools.lru_cache(maxsize=None)
def _runs(kind, packed, which="ragged", ss=0.0, fold=True):
    """{switch: (loss, flat gradients, bias gradients, step-0 state of the attention LSTM, column sums of dP1 / dP2)} of ONE model."""
    torch.manual_seed(0)
    m = models.setup(argparse.Namespace(**_opt(kind, ss))).to(DEV).train()
    batch = {k: v.to(DEV) for k, v in _batch(which).items()}
    real, res = ops.Recurrence, {}
    for on in (False, True):
        blocks = []

        class Spy(real):                    # keeps the tensors of both argument blocks (forward, backward) reachable
            def __init__(self, **fields):
                blocks.append(fields)
                super().__init__(**fields)

        ops.ZERO_STATE_SKIP, ops.Recurrence, F_.FOLD_BIAS_SUMS = on, Spy, fold
        try:
            m._dropout_calls = 0            # the same Philox stream for both runs
            m.packed_decoder = packed
            lw = models.LossWrapper(m, None)
            m.flatten_grads()
            b = batch
            out = lw(b["fc_feats"], b["att_feats"], b["labels"], b["masks"], b["att_masks"], None, None, None, b["obj_dist"], None, b["rel_ind"],
                     None, b["pred_dist"], b["gpn_obj_ind"], b["gpn_pred_ind"], b["gpn_nrel_ind"], b["gpn_pool_mtx"])
            models.total_loss(out).backward()
            torch.cuda.synchronize()
        finally:
            ops.ZERO_STATE_SKIP, ops.Recurrence, F_.FOLD_BIAS_SUMS = True, real, True
        g = m.flat_grads.clone()
        bias = {n: g[m._slots[n][0]:m._slots[n][0] + m._slots[n][1]].clone() for n in BIASES}
        step0 = sums = None
        fwd = [f for f in blocks if "H2" in f]
        bwd = [f for f in blocks if "dP1" in f]
        if fwd:
            f = fwd[0]
            assert f["zero_state"] == int(on)
            m0, R = f["m"][0], f["R"]
            H2 = f["H2"] if f["H2"].dim() == 2 else f["H2"][0]
            step0 = (f["G1"].reshape(-1, 4 * R)[:m0].clone(), f["C1"][1][:m0].clone(), H2[:m0, R:2 * R].float().clone())
        if bwd:
            f = bwd[0]
            assert f["zero_state"] == int(on)
            rows, R = f["row0"][f["T"]], f["R"]
            sums = tuple(ops.colsum(f[k].view(-1, 4 * R)[:rows]).clone() for k in ("dP1", "dP2"))
        res[on] = (float(out["lang_loss"].detach()), g, bias, step0, sums)
    res["slots"] = dict(m._slots)
    return res


def _close(a, b, top, bf, what=""):
    # fp32: tests/test_packed_gpu.py:47-49; bf16: tests/test_poison_gpu.py:58,63
    atol, rtol = (2e-3 * top, 2e-2) if bf else (2e-5 * top + 1e-7, 2e-4)
    np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), atol=atol, rtol=rtol, err_msg=what)


def _same_step(res, bf):
    (l0, g0, *_), (l1, g1, *_) = res[False], res[True]
    print(f"loss off {l0!r} on {l1!r}  max |dg| {float((g1 - g0).abs().max()):.3e}  max |g| {float(g0.abs().max()):.3e}")
    assert np.isfinite(l1) and bool(torch.isfinite(g1).all())
    assert abs(l0 - l1) <= (1e-3 if bf else 2e-5) * max(1.0, abs(l0))
    _close(g1, g0, float(g0.abs().max()), bf)


@pytest.mark.parametrize("kind", ["subgc_f32", "subgc_bf16", "fullgc_f32_dropout", "fullgc_bf16_shared"])
@pytest.mark.parametrize("packed", [True, False])
def test_switch_on_equals_switch_off(kind, packed):
    _same_step(_runs(kind, packed), "bf16" in kind)


def test_switch_on_equals_switch_off_under_scheduled_sampling():
    """sampling_prob > 0 takes the step-by-step Python loop, which issues the same launches as the C recurrence."""
    _same_step(_runs("subgc_f32", True, ss=0.25), False)


@pytest.mark.parametrize("kind", ["subgc_f32", "subgc_bf16"])
@pytest.mark.parametrize("packed", [True, False])
def test_attention_cell_of_step_0_only_loses_exact_zeros(kind, packed):
    """The attention LSTM's step-0 gates were (0 . Wc1^T) + x->gates + fc->gates + biases: without the product the same terms are added
    in the same order, so the gates, the cell state and h1_0 are the same numbers (torch.equal: signed zeros compare equal)."""
    res = _runs(kind, packed)
    for name, off, on in zip(("G1 rows of step 0", "C1[1]", "h1_0 columns of H2"), res[False][3], res[True][3]):
        assert off.numel() > 0 and bool(torch.isfinite(off).all()), name
        assert torch.equal(off, on), name


@pytest.mark.parametrize("which", ["no_words", "two_empty", "equal_len"])
@pytest.mark.parametrize("packed", [True, False])
def test_edge_batches(which, packed):
    _same_step(_runs("subgc_f32", packed, which), False)


def test_no_words_batch_has_one_step_and_no_row_after_it():
    """The `no_words` batch really is the K = 0 case of the cut weight gradients (packed decoder): one live step, rows == M[0]."""
    from subgc.functions_packed import live_plan
    b = _batch("no_words")
    _, M, _ = live_plan(b["labels"].to(DEV), b["masks"][:, 1:].to(DEV))
    assert M[0] == b["labels"].size(0) and sum(M) == M[0]
    # no row after step 0: the gradients of the weights that only ever met the zero state are exactly zero (the flat bucket starts zeroed
    # and the no-rows form of the weight gradient leaves what it accumulates into untouched)
    res = _runs("subgc_f32", True, "no_words")
    g, slots, R = res[True][1], res["slots"], OPT["rnn_size"]
    view = lambda n: g[slots[n][0]:slots[n][0] + slots[n][1]].view(slots[n][2])
    assert not bool(view("core.lang_lstm.weight_hh").any()) and not bool(view("core.att_lstm.weight_hh").any())
    assert not bool(view("core.att_lstm.weight_ih")[:, :R].any()) and bool(view("core.att_lstm.weight_ih")[:, R:].any())


@pytest.mark.parametrize("kind", ["subgc_f32", "subgc_bf16"])
@pytest.mark.parametrize("packed,which,fold", [(True, "ragged", True), (False, "ragged", True), (True, "two_empty", True), (True, "ragged", False)])
def test_bias_gradients_cover_every_row(kind, packed, which, fold):
    """With the switch on b_ih and b_hh of each LSTM get ONE set of column sums of dP1 / dP2 over ALL rows, the rows of step 0 included
    (a bias sum that rode one of the cut products would miss them); fold = False: the separate column-sum launches."""
    bf = "bf16" in kind
    res = _runs(kind, packed, which, fold=fold)
    off, on, sums = res[False][2], res[True][2], res[True][4]
    top = float(res[False][1].abs().max())
    for lstm, s in zip(("att", "lang"), sums):
        ih, hh = on[f"core.{lstm}_lstm.bias_ih"], on[f"core.{lstm}_lstm.bias_hh"]
        assert float(ih.abs().max()) > 0
        assert torch.equal(ih, hh), lstm
        _close(ih, s, top, bf, f"{lstm}: against the column sums of the saved gate gradients")
        _close(ih, off[f"core.{lstm}_lstm.bias_ih"], top, bf, f"{lstm}: against the switch-off run")
        _close(hh, off[f"core.{lstm}_lstm.bias_hh"], top, bf, f"{lstm}: against the switch-off run")
