"""CPU checks of subgc.optim (no GPU): the reference's parameter order and the parameters it skips, the build_optimizer surface, the
re-keying helpers, the state_dict format and its validation on load, and the host-side rejects of subgc_clip_optim_step."""
import argparse
import re

import pytest
import torch

from oracle import subgc_oracle as O
import subgc.models as models
from subgc import _lib, ops, optim

TRAIN = ["subgc_train", "fullgc_train", "subgc_gtsubg_train"]
RULES = ["adam", "adamw", "sgd", "sgdm", "sgdmom", "rmsprop", "adagrad"]


def _model(g):
    torch.manual_seed(0)
    m = models.setup(g.opt(caption_model="topdown", gpn_drop_prob=0.0))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in g.group("weights").items()})
    return m


def _opt(optim_name, lr=5e-4):
    return argparse.Namespace(optim=optim_name, learning_rate=lr, optim_alpha=0.9, optim_beta=0.999, optim_epsilon=1e-8, weight_decay=0.0)


@pytest.mark.parametrize("name", TRAIN)
def test_reference_param_names_follow_the_reference_state_dict(golden, name):
    """The golden weights are the reference's own state_dict(): its parameter keys, buffers removed, in file order."""
    g = golden(name)
    keys = [k for k in g.group("weights") if "running_" not in k and "num_batches" not in k]
    m = _model(g)
    assert optim.reference_param_names(m) == keys
    assert sorted(n for n, _ in m.named_parameters()) == sorted(keys)


@pytest.mark.parametrize("name", TRAIN)
def test_skipped_params_are_those_without_an_oracle_gradient(golden, name):
    g = golden(name)
    orc = O.Oracle(g.opt(gpn_drop_prob=0.0), g.group("weights"), requires_grad=True)
    orc.training = True
    r = O.loss_wrapper(orc, g.tensors("inputs"))
    (r["lang_loss"] + (r["gpn_loss"] if r["gpn_loss"] is not None else 0.0)).backward()
    none = [k for k, p in orc.P.items() if p.grad is None]
    assert len(none) == {"subgc_train": 19, "subgc_gtsubg_train": 19, "fullgc_train": 12}[name]
    assert optim.skipped_param_names(_model(g)) == none


@pytest.mark.parametrize("rule", RULES)
def test_build_optimizer_mirrors_the_reference(golden, rule):
    """misc/utils.py:223-239: the same torch class with the same hyperparameters; one group over the parameters in reference order."""
    m = _model(golden("subgc_train"))
    o = _opt(rule)
    fused = optim.build_optimizer(m, o)
    x = torch.zeros(1, requires_grad=True)
    want = {"rmsprop": lambda: torch.optim.RMSprop([x], o.learning_rate, o.optim_alpha, o.optim_epsilon, weight_decay=o.weight_decay),
            "adagrad": lambda: torch.optim.Adagrad([x], o.learning_rate, weight_decay=o.weight_decay),
            "sgd": lambda: torch.optim.SGD([x], o.learning_rate, weight_decay=5e-4, momentum=0.9),
            "sgdm": lambda: torch.optim.SGD([x], o.learning_rate, o.optim_alpha, weight_decay=o.weight_decay),
            "sgdmom": lambda: torch.optim.SGD([x], o.learning_rate, o.optim_alpha, weight_decay=o.weight_decay, nesterov=True),
            "adam": lambda: torch.optim.Adam([x], o.learning_rate, (o.optim_alpha, o.optim_beta), o.optim_epsilon, weight_decay=o.weight_decay),
            "adamw": lambda: torch.optim.AdamW([x], o.learning_rate, weight_decay=0.01)}[rule]()
    assert len(fused.param_groups) == 1
    grp = fused.param_groups[0]
    assert {k: v for k, v in grp.items() if k != "params"} == {k: v for k, v in want.param_groups[0].items() if k != "params"}
    assert [id(p) for p in grp["params"]] == [id(m.P(n)) for n in optim.reference_param_names(m)]
    for new_lr in (0.0, 1e-3):                                          # misc/utils.py:158-164 set_lr / get_lr
        for group in fused.param_groups:
            group["lr"] = new_lr
        assert next(iter(fused.param_groups))["lr"] == new_lr


def test_build_optimizer_rejects_an_unknown_name(golden):
    with pytest.raises(Exception, match="bad option opt.optim: lbfgs"):
        optim.build_optimizer(_model(golden("subgc_train")), _opt("lbfgs"))


def _torch_run(rule, params, steps=2, seed=0):
    """A torch optimizer of `rule` over `params` after `steps` steps on random gradients (skipped parameters keep grad None)."""
    o = _opt(rule, lr=1e-2)
    cls = {"adam": lambda p: torch.optim.Adam(p, o.learning_rate, (0.9, 0.999), 1e-8), "adamw": lambda p: torch.optim.AdamW(p, o.learning_rate, weight_decay=0.01),
           "sgd": lambda p: torch.optim.SGD(p, o.learning_rate, weight_decay=5e-4, momentum=0.9),
           "rmsprop": lambda p: torch.optim.RMSprop(p, o.learning_rate, 0.9, 1e-8), "adagrad": lambda p: torch.optim.Adagrad(p, o.learning_rate)}[rule]
    opt = cls([p for _, p in params])
    gen = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        for live, p in params:
            p.grad = torch.randn(p.shape, generator=gen) if live else None
        opt.step()
    return opt


@pytest.mark.parametrize("rule", ["adam", "adamw", "sgd", "rmsprop", "adagrad"])
def test_state_dict_round_trip_through_the_fused_format(golden, rule):
    """A torch state_dict over the reference order (skipped parameters without gradients) loads into the fused optimizer and comes
    back out identical: keys, step counts, tensors and hyperparameters."""
    g = golden("subgc_train")
    m = _model(g)
    skipped = set(optim.skipped_param_names(m))
    names = optim.reference_param_names(m)
    params = [(n not in skipped, torch.nn.Parameter(m.P(n).detach().clone())) for n in names]
    sd = _torch_run(rule, params).state_dict()
    fused = optim.build_optimizer(m, _opt(rule))
    fused.load_state_dict(sd)
    if rule != "sgd":
        assert fused.t == 2
    out = fused.state_dict()
    assert sorted(out["state"]) == sorted(sd["state"])
    for i, e in sd["state"].items():
        assert sorted(out["state"][i]) == sorted(e), names[i]
        for k, v in e.items():
            if torch.is_tensor(v):
                assert torch.equal(out["state"][i][k], v), (names[i], k)
            else:
                assert out["state"][i][k] == v
    assert {k: v for k, v in out["param_groups"][0].items() if k != "params"} == \
        {k: v for k, v in sd["param_groups"][0].items() if k != "params"}
    assert out["param_groups"][0]["params"] == list(range(len(names)))
    if rule == "adagrad":                                               # Adagrad: every parameter has an entry, skipped ones at step 0
        assert all(float(out["state"][names.index(n)]["step"]) == 0.0 for n in skipped)
    else:
        assert not any(names.index(n) in out["state"] for n in skipped)


def test_load_takes_int_steps_and_the_files_hyperparameters(golden):
    m = _model(golden("subgc_train"))
    skipped = set(optim.skipped_param_names(m))
    params = [(n not in skipped, torch.nn.Parameter(m.P(n).detach().clone())) for n in optim.reference_param_names(m)]
    sd = _torch_run("adam", params, steps=3).state_dict()
    for e in sd["state"].values():
        e["step"] = int(e["step"])                                      # the reference's torch stored ints
    sd["param_groups"][0]["lr"] = 1.25e-4
    fused = optim.build_optimizer(m, _opt("adam"))
    fused.load_state_dict(sd)
    assert fused.t == 3 and fused.param_groups[0]["lr"] == 1.25e-4
    assert all(float(e["step"]) == 3.0 for e in fused.state_dict()["state"].values())


def test_load_rejects_mixed_step_counts(golden):
    m = _model(golden("subgc_train"))
    skipped = set(optim.skipped_param_names(m))
    params = [(n not in skipped, torch.nn.Parameter(m.P(n).detach().clone())) for n in optim.reference_param_names(m)]
    sd = _torch_run("adam", params).state_dict()
    first = min(sd["state"])
    sd["state"][first]["step"] = torch.tensor(7.0)
    fused = optim.build_optimizer(m, _opt("adam"))
    with pytest.raises(ValueError, match="different step counts"):
        fused.load_state_dict(sd)
    sd = _torch_run("adam", params).state_dict()
    del sd["state"][first]                                              # a live parameter without state beside ones with it
    with pytest.raises(ValueError, match="live parameters"):
        fused.load_state_dict(sd)


def test_adagrad_file_with_step0_skipped_entries_loads(golden):
    m = _model(golden("subgc_train"))
    names = optim.reference_param_names(m)
    skipped = set(optim.skipped_param_names(m))
    params = [(n not in skipped, torch.nn.Parameter(m.P(n).detach().clone())) for n in names]
    sd = _torch_run("adagrad", params, steps=4).state_dict()
    assert all(float(sd["state"][names.index(n)]["step"]) == 0.0 for n in skipped) and len(sd["state"]) == len(names)
    fused = optim.build_optimizer(m, _opt("adagrad"))
    fused.load_state_dict(sd)
    assert fused.t == 4


def test_rekeying_helpers_move_a_torch_state_between_the_two_orders(golden):
    m = _model(golden("fullgc_train"))
    own = [n for n, _ in m.named_parameters()]
    ref = optim.reference_param_names(m)
    assert own != ref                                                   # the decoder's modules are ordered differently
    params = [(True, torch.nn.Parameter(m.P(n).detach().clone())) for n in own]
    sd = _torch_run("adam", params).state_dict()
    r = optim.state_dict_to_reference(m, sd)
    for j, n in enumerate(ref):
        assert torch.equal(r["state"][j]["exp_avg"], sd["state"][own.index(n)]["exp_avg"]), n
    back = optim.state_dict_from_reference(m, r)
    assert sorted(back["state"]) == sorted(sd["state"])
    assert all(torch.equal(back["state"][i]["exp_avg_sq"], sd["state"][i]["exp_avg_sq"]) for i in sd["state"])
    # what the helper prevents: the reference-keyed file pairs a moment with a parameter of another shape under the project's order
    assert any(r["state"][i]["exp_avg"].shape != p.shape for i, (_, p) in enumerate(params))


def test_optim_rules_match_the_header():
    src = open(_lib.HEADER).read()
    defs = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define\s+SUBGC_OPTIM_(\w+)\s+(\d+)", src)}
    assert defs == ops.OPTIM_RULES
    protos = _lib.parse_header()
    assert "subgc_clip_optim_step" in protos and "subgc_clip_optim_step_zero" in protos


@pytest.mark.parametrize("zero", [False, True])
@pytest.mark.parametrize("args,what", [
    (dict(rule=7), b"unknown rule"),
    (dict(step=0), b"bad arguments"),
    (dict(n_live=-1), b"bad arguments"),
    (dict(lr=-1.0), b"bad hyperparameters"),
    (dict(rule=0, h0=1.0), b"betas"),
    (dict(rule=2, flags=1, h0=0.9, h1=0.1), b"Nesterov"),
    (dict(rule=0, flags=1), b"SGD option"),
    (dict(rule=1, s2=None), b"null pointer"),
    (dict(n_live=2, live=None), b"null pointer"),
])
def test_clip_optim_step_rejects_on_the_host(zero, args, what):
    L = _lib.lib()
    fake = 1 << 20                                                      # never dereferenced: the checks come first
    a = dict(rule=0, p=fake, g=fake, s1=fake, s2=fake, n=1024, live=None, n_live=0, sumsq=fake, max_norm=10.0, grad_scale=1.0, lr=1e-3,
             h0=0.9, h1=0.999, eps=1e-8, wd=0.0, step=1, flags=0, p16=None, stream=None)
    a.update(args)
    fn = L.subgc_clip_optim_step_zero if zero else L.subgc_clip_optim_step
    rc = fn(a["rule"], a["p"], a["g"], a["s1"], a["s2"], a["n"], a["live"], a["n_live"], a["sumsq"], a["max_norm"], a["grad_scale"], a["lr"],
            a["h0"], a["h1"], a["eps"], a["wd"], a["step"], a["flags"], a["p16"], a["stream"])
    assert rc == -1
    err = L.subgc_last_error()
    assert b"clip_optim_step" in err and what in err, err
