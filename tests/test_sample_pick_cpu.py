"""CPU side of top-k sampling at any the_k and of the nucleus option the_p: the oracle is pinned against the reference's own sampled
path at the_k = 10 (golden case subgc_topk10, written by tests/golden/make_golden_topk.py), and the model refuses option values the
sampler cannot serve when it is built."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

from oracle import subgc_oracle as O
from subgc import synthetic
import subgc.models as models

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def topk10_case(golden):
    """The subgc_topk10 case: its settings live in a meta file of their own (meta.json is not rewritten for it)."""
    g = golden("subgc_topk10")
    with open(os.path.join(GOLDEN, "subgc_topk10_meta.json")) as f:
        g.meta = json.load(f)["subgc_topk10"]
    return g


def test_topk10_reference_path_pinned(golden):
    """The oracle forced along the reference's sampled path at the_k = 10: every live token lies in the oracle's top-10 of its step with
    the reference's log-prob (1e-4: the fixture tolerance of meta.json), and the kept sub-graphs are the reference's."""
    g = topk10_case(golden)
    assert g.meta["opt"]["the_k"] == 10 and g.meta["opt"]["use_topk_sampling"] == 1
    with open(os.path.join(GOLDEN, "meta.json")) as f:
        tol = json.load(f)["tolerances"]["fp32_atol"]
    assert tol == 1e-4
    ref = g.group("out")
    same_inputs = golden("subgc_topk").group("inputs")
    for k, v in g.group("inputs").items():
        np.testing.assert_array_equal(v, same_inputs[k])
    orc = O.Oracle(g.opt(), golden("subgc_train").group("weights"))
    tap = {}
    ret = orc.sample(*synthetic.sample_args(g.tensors("inputs")), opt=g.meta["sample_opt"], forced=torch.from_numpy(ref["seq"]), tap=tap)
    np.testing.assert_array_equal(ret[3].numpy(), ref["keep_ind"])
    steps = ref["step_logp"].shape[0]
    np.testing.assert_allclose(torch.stack(tap["step_logp"][:steps], 0).numpy(), ref["step_logp"], atol=tol, rtol=2e-5)
    seq, lps = ref["seq"], ref["seqLogprobs"]
    alive = np.ones(seq.shape[0], bool)
    checked = beyond3 = 0
    for t in range(min(steps, seq.shape[1])):
        idx = tap["topk_idx"][t].numpy(); top = tap["topk_lp"][t].numpy()
        assert idx.shape[1] == 10
        for r in range(seq.shape[0]):
            if alive[r] and seq[r, t] > 0:
                j = np.where(idx[r] == seq[r, t])[0]
                assert len(j) == 1, (r, t)
                assert abs(top[r, j[0]] - lps[r, t]) < tol
                checked += 1
                beyond3 += j[0] >= 3
        alive &= seq[:, t] > 0
    assert checked > 50
    assert beyond3 > 0                                                           # the path really needs the wider k


@pytest.mark.parametrize("over", [dict(the_k=0), dict(the_k=52), dict(the_p=0.0), dict(the_p=1.5)])
def test_sampler_options_out_of_range_are_refused_at_construction(golden, over):
    g = golden("subgc_train")
    assert g.meta["opt"]["vocab_size"] == 50                                     # the_k = 52 = vocab_size + 2
    with pytest.raises(ValueError, match="the_k|the_p"):
        models.setup(g.opt(caption_model="topdown", use_topk_sampling=1, **over))


def test_sampler_options_in_range_are_accepted(golden):
    g = golden("subgc_train")
    m = models.setup(g.opt(caption_model="topdown", use_topk_sampling=1, the_k=51, the_p=0.9))      # the whole logit row
    assert m.the_k == 51 and m.the_p == 0.9
    m = models.setup(g.opt(caption_model="topdown", use_topk_sampling=1, the_k=1))
    assert m.the_k == 1 and m.the_p == 1.0
    # without top-k sampling the options are not read by any decode path and are left alone
    assert models.setup(g.opt(caption_model="topdown", the_k=0)).topk_sampling is False
