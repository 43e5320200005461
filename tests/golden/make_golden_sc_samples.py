#!/usr/bin/env python
"""Golden vectors of the one-pass self-critical step (n samples per caption row, leave-one-out baseline), produced by RUNNING THE
REFERENCE's own code on the CPU -- `RewardCriterion` of misc/utils.py:89-109, the COCO scorers of misc/coco-caption/pycocoevalcap and the
reference model -- imported from where the reference lies, never copied.  Two files of data:

sc_samples_case.npz
    for n in {2, 3, 5}: fixed token rows [n * 4, L] (sample-major: row k * 4 + s is sample k of caption row s) of 4 caption rows over 2
    images -- among them a row that ends at step 0, a row without an end token and two identical samples in one group --, their CIDEr /
    BLEU-4 from the reference's scorers, the scores w_cider * CIDEr + w_bleu * BLEU-4, the rewards and baselines of the contract
    (subgc.selfcritical.loo_reward_restatement on those scores) and the loss of the reference's RewardCriterion on seeded
    log-probabilities with those rewards.
sc_samples_train.npz
    the reference MODEL on the subgc_train and fullgc_train golden weights and inputs (dropout 0), teacher-forced along fixed token rows
    [n * b5, T] for n = 2 and 3 -- one forward per sample block, the encoder's gradient summed over the blocks as the one-pass step sums
    it -- with the objective RewardCriterion()(gathered log-probabilities of ALL n * b5 rows, tokens, leave-one-out rewards) + gpn_loss.
    Stored per case under the prefix '<model>.n<n>.': the tokens, the references, the scores and rewards, lang_loss / gpn_loss / loss and
    the gradient of every live parameter -- in full up to 4096 entries, else 1024 seeded entries and the norm
    (tests/sc_samples_golden.py: a committed file is limited to 1 MiB).

    python tests/golden/make_golden_sc_samples.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  (helpers only: ref_opt, build, enter_scratch, np_)
import make_golden_self_critical as SC  # noqa: E402  (array_to_str, score_rows, random_caption, write_npz, the reward weights)
import sc_samples_golden as SG  # noqa: E402
from subgc.selfcritical import loo_reward_restatement  # noqa: E402

L, V, ROWS, N_IMG = 9, 14, 4, 2


def perturbed(rng, refs_j, width, vocab, cut=0.4):
    row = refs_j[int(rng.integers(0, len(refs_j)))].copy()
    n = int((row > 0).sum())
    for _ in range(int(rng.integers(0, 4))):
        row[int(rng.integers(0, n))] = rng.integers(1, vocab + 1)
    if rng.random() < cut and n > 2:
        row[int(rng.integers(1, n)):] = 0
    return row


def loo(scores, n):
    reward, baseline, mean = loo_reward_restatement(scores, n)
    return reward, baseline, np.float64(mean)


def case_file(RewardCriterion, Bleu, Cider):
    rng = np.random.default_rng(20271)
    refs = [np.stack([SC.random_caption(rng, int(rng.integers(3, L + 1)), L, V) for _ in range(2 + j)]) for j in range(N_IMG)]
    img_of_row = np.array([0, 0, 1, 1], np.int64)                      # caption row s belongs to image s // 2
    out = {"ref_rows": np.concatenate(refs), "ref_cap_off": np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.int64),
           "img_of_row": img_of_row, "weights": np.array([SC.W_CIDER, SC.W_BLEU])}
    gen = torch.Generator().manual_seed(20272)
    for n in SG.NS_CASE:
        tok = np.stack([perturbed(rng, refs[int(img_of_row[r % ROWS])], L, V) for r in range(n * ROWS)])
        tok[0] = 0                                                     # sample 0 of caption row 0 ends at step 0
        tok[ROWS + 1] = rng.integers(1, V + 1, L)                      # sample 1 of caption row 1 has no end token
        tok[(n - 1) * ROWS + 2] = tok[2]                               # caption row 2: its last sample equals its first
        tok[3] = refs[1][0]                                            # a sample equal to a reference
        bleu, cider = SC.score_rows(Bleu, Cider, refs, tok, np.tile(img_of_row, n))
        scores = SC.W_CIDER * cider + SC.W_BLEU * bleu[:, 3]
        reward, baseline, mean = loo(scores, n)
        logp = -torch.rand(n * ROWS, L + 1, generator=gen) * 5.0 - 0.01
        seq = torch.zeros(n * ROWS, L + 1, dtype=torch.long)
        seq[:, :L] = torch.from_numpy(tok)                             # the criterion's own view: the row and its closing 0
        rw = torch.from_numpy(reward).view(-1, 1).expand(n * ROWS, L + 1)
        loss = RewardCriterion()(logp, seq, rw)
        out.update({f"n{n}.tok": tok, f"n{n}.bleu": bleu, f"n{n}.cider": cider, f"n{n}.scores": scores, f"n{n}.reward": reward,
                    f"n{n}.baseline": baseline, f"n{n}.mean_reward": mean, f"n{n}.logp": MG.np_(logp), f"n{n}.loss": MG.np_(loss)})
    SC.write_npz(os.path.join(HERE, "sc_samples_case.npz"), out)


def train_case(RewardCriterion, Bleu, Cider, name, opt, out):
    import json
    from subgc import synthetic
    with open(os.path.join(HERE, "meta.json")) as f:
        base = json.load(f)[name]
    with np.load(os.path.join(HERE, name + "_weights.npz")) as z:
        weights = {k: z[k] for k in z.files}
    with np.load(os.path.join(HERE, name + "_inputs.npz")) as z:
        batch = {k: torch.from_numpy(z[k]) for k in z.files}
    b5, Tm, Vm, B = batch["labels"].size(0), batch["labels"].size(1) - 2, MG.TINY["vocab_size"], base["B"]
    spi = b5 // B
    gt_indices = np.array([2, 0, 1], np.int64)
    for n in SG.NS_TRAIN:
        model = MG.build(opt, base["seed"], base["gcn_scale"])
        for k, v in model.state_dict().items():
            assert np.array_equal(MG.np_(v), weights[k]), k                 # the construction of the golden case: no second weight file
        model.train()
        rng = np.random.default_rng(20273 + n)
        refs = [np.stack([SC.random_caption(rng, int(rng.integers(3, Tm + 1)), Tm, Vm) for _ in range(2 + j)]) for j in range(B)]
        img_of_row = np.tile(gt_indices[np.arange(b5) // spi], n)
        tok = np.stack([perturbed(rng, refs[int(img_of_row[r])], Tm, Vm) for r in range(n * b5)])
        tok[4] = 0                                                      # an empty sample
        tok[b5 + 6] = rng.integers(1, Vm + 1, Tm)                       # a full-length one
        tok[(n - 1) * b5 + 9] = tok[9]                                  # two identical samples in one group
        bleu, cider = SC.score_rows(Bleu, Cider, refs, tok, img_of_row)
        scores = SC.W_CIDER * cider + SC.W_BLEU * bleu[:, 3]
        reward, baseline, mean = loo(scores, n)
        gathered, gpn_loss = [], None
        for k in range(n):
            seq = torch.from_numpy(tok[k * b5:(k + 1) * b5])
            labels = torch.zeros(b5, Tm + 2, dtype=torch.long)
            labels[:, 1:Tm + 1] = seq
            fed = {key: v.clone() for key, v in batch.items()}
            fed["labels"] = labels
            outputs, gpn_k, _ = model(*synthetic.forward_args(fed))
            gathered.append(outputs[:, :Tm].gather(2, seq.unsqueeze(2)).squeeze(2))
            gpn_loss = gpn_k if gpn_loss is None else gpn_loss          # the same number in every pass: it does not read the labels
        rw = torch.from_numpy(reward).view(-1, 1).expand(n * b5, Tm)
        lang_loss = RewardCriterion()(torch.cat(gathered), torch.from_numpy(tok), rw)
        loss = lang_loss + (gpn_loss if gpn_loss is not None else 0.0)
        loss.backward()
        pre = f"{name}.n{n}."
        out.update({pre + "lang_loss": MG.np_(lang_loss), pre + "loss": MG.np_(loss), pre + "sc.tok": tok, pre + "sc.ref_rows": np.concatenate(refs),
                    pre + "sc.ref_cap_off": np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.int64),
                    pre + "sc.gt_indices": gt_indices, pre + "sc.weights": np.array([SC.W_CIDER, SC.W_BLEU]), pre + "sc.scores": scores,
                    pre + "sc.reward": reward, pre + "sc.baseline": baseline, pre + "sc.mean_reward": mean})
        if gpn_loss is not None:
            out[pre + "gpn_loss"] = MG.np_(gpn_loss)
        for k, p in model.named_parameters():
            if p.grad is not None:
                for key, v in SG.stored_gradient(k, MG.np_(p.grad)).items():
                    out[pre + "grad." + key] = v


def main():
    assert os.path.isdir(MG.REF), "golden vectors can only be regenerated where the reference exists"
    MG.enter_scratch()
    from misc.utils import RewardCriterion
    Bleu, Cider = SC.scorers()
    case_file(RewardCriterion, Bleu, Cider)
    out = {}
    train_case(RewardCriterion, Bleu, Cider, "subgc_train", MG.ref_opt(), out)
    fo = dict(use_gpn=0, noun_fuse=0, pred_emb_type=2, gcn_layers=4, gcn_residual=1, gcn_bn=1)        # make_golden.py's Full-GC case
    train_case(RewardCriterion, Bleu, Cider, "fullgc_train", MG.ref_opt(**fo), out)
    SC.write_npz(os.path.join(HERE, "sc_samples_train.npz"), out)


if __name__ == "__main__":
    main()
