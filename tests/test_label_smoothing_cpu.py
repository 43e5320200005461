"""The label-smoothed language loss without a GPU: the fifth header and its binding, the fixture the reference's own LabelSmoothing wrote
(tests/golden/make_golden_label_smoothing.py) against the fp64 restatement of the closed form that the GPU tests use as their reference,
and the host-side validation of `smoothing` and of LossWrapper's choice of criterion."""
import argparse
import ctypes

import numpy as np
import pytest

import label_smoothing_golden as G
from subgc import _lib, ops
from subgc._lib import SubgcError
import subgc.models as models

NAMES = {
    "subgc_row_lse_sum_f32": ["x", "ldx", "rows", "V", "lse", "slp", "stream"],
    "subgc_smoothed_nll_fwd": ["logp", "target", "t_stride", "mask", "m_stride", "slp", "smoothing", "loss", "scratch2", "S", "T", "V",
                               "den_override", "lse", "stream"],
    "subgc_smoothed_nll_bwd": ["target", "t_stride", "mask", "m_stride", "scratch2", "dloss", "smoothing", "dlogp", "S", "T", "V", "stream"],
    "subgc_smoothed_logsoftmax_bwd": ["logp", "target", "t_stride", "mask", "m_stride", "scratch2", "dloss", "smoothing", "dlogits", "ld_out",
                                      "S", "T", "V", "active", "out_bf16", "lse", "stream"],
}


def test_criterion_header_parses_and_the_other_four_are_untouched():
    protos = _lib.parse_header(_lib.CRITERION_HEADER)
    assert sorted(protos) == sorted(NAMES)
    for name, want in NAMES.items():
        ret, args = protos[name]
        assert ret is ctypes.c_int and [a for _, a in args] == want, name
        assert dict((a, t) for t, a in args)["stream"] is ctypes.c_void_p
        if "smoothing" in want:
            assert args[want.index("smoothing")][0] is ctypes.c_double
    # the fused backward = subgc_nll_logsoftmax_bwd's arguments plus `smoothing`
    core = _lib.parse_header()
    assert [a for a in NAMES["subgc_smoothed_logsoftmax_bwd"] if a != "smoothing"] == [a for _, a in core["subgc_nll_logsoftmax_bwd"][1]]
    src = open(_lib.CRITERION_HEADER).read()
    assert src.count("misc/utils.py:126-156") >= 5                                               # the file and every entry cite the class


def test_closed_form_reproduces_the_reference_class():
    """fp64 numpy closed form against what misc/utils.py:126-156 computed in fp32 (KLDivLoss on the dense true_dist): the loss to fp32
    rounding of a 15-row sum of 37-term rows, the gradient to two fp32 roundings.  Every later closed-form check leans on this one."""
    meta, arr = G.load_case()
    assert (meta["S"], meta["T"], meta["V"]) == arr["logp"].shape == (3, 5, 37) and arr["target"].shape == arr["mask"].shape == (3, 7)
    tgt, msk = arr["target"][:, :5], arr["mask"][:, :5]
    assert tgt.min() == 0 and tgt.max() == 36 and not msk[1].any() and msk[0, 2] == 0 and msk[0, 1] == msk[0, 3] == 1
    assert not arr["logp"][0, 4].any() and msk[0, 4] == 1 and not arr["logp"][2, 4].any() and msk[2, 4] == 0     # the two zero rows
    assert meta["smoothings"] == [0.0, 0.1, 0.5, 1.0]
    for s, key in zip(meta["smoothings"], meta["keys"]):
        loss, dlogp = G.closed_form(arr["logp"], arr["target"], arr["mask"], s)
        assert abs(loss - float(arr["loss_" + key])) <= G.loss_bound(arr["logp"], arr["target"], arr["mask"], s) + 8 * G.U * abs(loss), s
        np.testing.assert_allclose(arr["dlogp_" + key], dlogp, rtol=4 * G.U, atol=0, err_msg=str(s))
        assert arr["dlogp_" + key].shape == (3, 5, 37)
    # the masked-in zero row is what separates the criteria: it adds nothing under NLL (s = 0) and m * H under smoothing
    conf, e, H = G.constants(0.1, 37)
    with_row, _ = G.closed_form(arr["logp"], arr["target"], arr["mask"], 0.1)
    m2 = arr["mask"].copy(); m2[0, 4] = 0
    without, _ = G.closed_form(arr["logp"], arr["target"], m2, 0.1)
    assert abs(with_row * float(arr["mask"][:, :5].sum()) - without * float(m2[:, :5].sum()) - H) < 1e-12 and H < -0.5


def test_train_fixture_holds_losses_and_every_live_gradient(golden):
    z, base = G.load_train(), golden("subgc_train")
    grads = base.group("grads")
    assert set(z) == set(grads) | {"lang_loss", "gpn_loss", "loss"}
    assert all(z[k].shape == grads[k].shape and z[k].dtype == np.float32 for k in grads)
    out = base.group("out")
    assert float(z["gpn_loss"]) == float(out["gpn_loss"]) and float(z["lang_loss"]) != float(out["lang_loss"])     # only the language loss changed
    assert abs(float(z["lang_loss"]) + float(z["gpn_loss"]) - float(z["loss"])) < 1e-6
    assert not np.array_equal(z["logit.weight"], grads["logit.weight"])


@pytest.mark.parametrize("bad", [-0.1, 1.5, float("nan"), float("inf")])
def test_bad_smoothing_is_refused_with_its_value(bad):
    shown = repr(float(bad))
    with pytest.raises(SubgcError) as e:
        ops.check_smoothing(bad)
    assert shown in str(e.value) and "[0, 1]" in str(e.value)
    with pytest.raises(SubgcError) as e:
        models.LabelSmoothing(smoothing=bad)
    assert shown in str(e.value)
    with pytest.raises(SubgcError) as e:
        models.LossWrapper(None, argparse.Namespace(label_smoothing=bad))
    assert shown in str(e.value)
    # the library refuses it on the host before it looks at any pointer (nothing is launched: no device needed)
    fwd = dict.fromkeys(NAMES["subgc_smoothed_nll_fwd"])
    fwd.update(t_stride=1, m_stride=1, smoothing=bad, S=1, T=1, V=5)
    bwd = dict.fromkeys(NAMES["subgc_smoothed_nll_bwd"])
    bwd.update(t_stride=1, m_stride=1, smoothing=bad, S=1, T=1, V=5)
    fused = dict.fromkeys(NAMES["subgc_smoothed_logsoftmax_bwd"])
    fused.update(t_stride=1, m_stride=1, smoothing=bad, ld_out=5, S=1, T=1, V=5, out_bf16=0)
    for name, a in (("subgc_smoothed_nll_fwd", fwd), ("subgc_smoothed_nll_bwd", bwd), ("subgc_smoothed_logsoftmax_bwd", fused)):
        with pytest.raises(SubgcError) as e:
            _lib.call_criterion(name, *a.values())
        assert f"smoothing {bad:g} is outside [0, 1]" in str(e.value), name
    assert ops.check_smoothing(0) == 0.0 and ops.check_smoothing(1) == 1.0 and ops.check_smoothing(0.1) == 0.1


def test_loss_wrapper_keeps_the_plain_criterion_unless_the_option_is_positive():
    for opt in (None, argparse.Namespace(), argparse.Namespace(label_smoothing=0), argparse.Namespace(label_smoothing=0.0),
                argparse.Namespace(label_smoothing=None)):
        lw = models.LossWrapper(None, opt)
        assert type(lw.crit) is models.LanguageModelCriterion and lw.label_smoothing == 0.0
    lw = models.LossWrapper(None, argparse.Namespace(label_smoothing=0.1))
    assert type(lw.crit) is models.LabelSmoothing and lw.crit.smoothing == 0.1 and lw.label_smoothing == 0.1
    crit = models.LabelSmoothing(size=0, padding_idx=0, smoothing=0.25)                          # the reference's constructor signature
    assert crit.smoothing == 0.25 and crit.confidence == 0.75
