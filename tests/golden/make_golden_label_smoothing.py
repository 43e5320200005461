#!/usr/bin/env python
"""Golden vectors of the label-smoothed language loss, produced by RUNNING THE REFERENCE's own class (CPU, fp32):
`LabelSmoothing` of misc/utils.py:126-156, imported from where the reference lies, never copied.  Two files of data:

label_smoothing_case.npz + label_smoothing_meta.json
    the class alone on small seeded inputs (S = 3, T = 5, V = 37) for smoothing in {0, 0.1, 0.5, 1.0}.  Target and mask are wider than T
    (the class truncates them), targets include 0 and V - 1, one sentence is fully masked, one mask has a zero in mid-sentence, and two
    rows of the input are zero as the reference's teacher-forced loop leaves them after its early break (AttModel.py:171-172), one of
    them masked in and one masked out.  Stored: the inputs, and per smoothing the loss and the gradient with respect to the input.
label_smoothing_train.npz
    the reference MODEL on the existing subgc_train golden inputs and weights (dropout 0, like that case) with the objective
    LabelSmoothing(smoothing=0.1)(lang_output, labels[:, 1:], masks[:, 1:]) + gpn_loss.  Stored: the losses and the gradient of every
    live parameter under its own name.

    python tests/golden/make_golden_label_smoothing.py
"""
import io
import json
import os
import sys
import warnings
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (helpers only: ref_opt, build, enter_scratch, np_)

SMOOTHINGS = [0.0, 0.1, 0.5, 1.0]
S, T, V, WIDE = 3, 5, 37, 7


def case_inputs():
    gen = torch.Generator().manual_seed(20260)
    logp = torch.log_softmax(torch.randn(S, T, V, generator=gen) * 3.0, dim=2)
    target = torch.randint(1, V - 1, (S, WIDE), generator=gen)
    target[0, 0], target[0, 1], target[2, 2] = 0, V - 1, 0
    mask = torch.ones(S, WIDE)
    mask[1] = 0.0                      # a fully masked sentence
    mask[0, 2] = 0.0                   # a zero in mid-sentence
    mask[2, 4] = 0.0                   # the masked-out zero row below
    logp[0, 4] = 0.0                   # rows left at zero after an early break: masked in ...
    logp[2, 4] = 0.0                   # ... and masked out
    return logp, target, mask


def criterion_case(LabelSmoothing):
    logp, target, mask = case_inputs()
    out = dict(logp=MG.np_(logp), target=target.numpy(), mask=mask.numpy())
    for s in SMOOTHINGS:
        x = logp.clone().requires_grad_(True)
        loss = LabelSmoothing(smoothing=s)(x, target, mask)
        loss.backward()
        key = f"s{int(round(s * 100)):03d}"
        out[f"loss_{key}"], out[f"dlogp_{key}"] = MG.np_(loss), MG.np_(x.grad)
    np.savez_compressed(os.path.join(HERE, "label_smoothing_case.npz"), **out)
    meta = dict(S=S, T=T, V=V, wide=WIDE, smoothings=SMOOTHINGS, keys=[f"s{int(round(s * 100)):03d}" for s in SMOOTHINGS],
                zero_rows=[[0, 4], [2, 4]], masked_sentence=1, mid_zero=[0, 2], source="misc/utils.py:126-156 (LabelSmoothing), fp32, CPU")
    with open(os.path.join(HERE, "label_smoothing_meta.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)


def train_case(LabelSmoothing):
    from subgc import synthetic
    with open(os.path.join(HERE, "meta.json")) as f:
        base = json.load(f)["subgc_train"]
    model = MG.build(MG.ref_opt(), base["seed"], base["gcn_scale"])
    with np.load(os.path.join(HERE, "subgc_train_weights.npz")) as z:
        for k, v in model.state_dict().items():
            assert np.array_equal(MG.np_(v), z[k]), k                    # same construction as subgc_train: no second weight file
    model.train()
    with np.load(os.path.join(HERE, "subgc_train_inputs.npz")) as z:
        batch = {k: torch.from_numpy(z[k]) for k in z.files}
    outputs, gpn_loss, score = model(*synthetic.forward_args({k: v.clone() for k, v in batch.items()}))
    lang_loss = LabelSmoothing(smoothing=0.1)(outputs, batch["labels"][:, 1:], batch["masks"][:, 1:])
    loss = lang_loss + gpn_loss
    loss.backward()
    out = {"lang_loss": MG.np_(lang_loss), "gpn_loss": MG.np_(gpn_loss), "loss": MG.np_(loss)}
    out.update({k: MG.np_(p.grad) for k, p in model.named_parameters() if p.grad is not None})      # every other key is a parameter's name
    # an .npz like np.savez_compressed writes it, deflated at the highest level: the file stays no larger than subgc_train_grads.npz
    with zipfile.ZipFile(os.path.join(HERE, "label_smoothing_train.npz"), "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for k, v in out.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(v), allow_pickle=False)
            zf.writestr(k + ".npy", buf.getvalue())


def main():
    assert os.path.isdir(MG.REF), "golden vectors can only be regenerated where the reference exists"
    MG.enter_scratch()
    warnings.simplefilter("ignore")                                      # the class passes KLDivLoss its deprecated size_average / reduce
    from misc.utils import LabelSmoothing
    criterion_case(LabelSmoothing)
    train_case(LabelSmoothing)


if __name__ == "__main__":
    main()
