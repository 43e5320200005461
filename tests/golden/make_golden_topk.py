#!/usr/bin/env python3
"""Add the top-k sampling case at the_k = 10 by RUNNING THE REFERENCE (CPU, fp32), without rewriting any other fixture.

    python tests/golden/make_golden_topk.py       # writes subgc_topk10_{inputs,out}.npz + subgc_topk10_meta.json

Same weights (subgc_train), seed and M as `subgc_topk`; only the_k differs, so the inputs equal that case's.  The case's settings
go to a meta file of its own: meta.json and every existing fixture stay byte-identical.  Runs only where make_golden.py runs.
"""
import json
import os

import numpy as np
import torch

import make_golden as mg


def main():
    assert os.path.isdir(mg.REF), "golden vectors can only be regenerated where the reference exists"
    mg.enter_scratch()
    torch.set_num_threads(1)
    with np.load(os.path.join(mg.HERE, "subgc_train_weights.npz")) as z:
        w = {k: z[k] for k in z.files}
    meta = {}
    t = dict(test_LSTM=1, gpn_nms_thres=0.75, gpn_max_subg=10)
    mg.run_sample("subgc_topk10", mg.ref_opt(**dict(t, use_topk_sampling=1, topk_temp=0.6, the_k=10)), w, seed=5, M=12,
                  sample_opt=dict(sample_max=1, beam_size=1), meta=meta)
    with open(os.path.join(mg.HERE, "subgc_topk10_meta.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True, default=str)
    print("golden written: subgc_topk10_inputs.npz subgc_topk10_out.npz subgc_topk10_meta.json")


if __name__ == "__main__":
    main()
