#!/usr/bin/env python
"""Golden vectors of self-critical sequence training, produced by RUNNING THE REFERENCE's own code (CPU): `RewardCriterion` of
misc/utils.py:89-109 and the COCO scorers of misc/coco-caption/pycocoevalcap, imported from where the reference lies, never copied.
Two files of data (plus a small meta file):

self_critical_case.npz + self_critical_meta.json
    (a) the class alone on small seeded inputs (S = 3, T = 5): one row of `seq` all zeros, one without a zero, rewards that are negative,
        zero and per-token, each with and without `gpn_loss`.  Stored: the inputs and per case the loss, d input and d gpn_loss.
    (b) `Cider().compute_score` and `Bleu(4).compute_score` of 2 x 20 candidate rows (a "sampled" and a "greedy" half) against 12 images
        with 1-5 reference captions each.  The strings are built as the upstream array_to_str builds them -- the decimal ids, the end
        token 0 included as a word, nothing after it; a row without a 0 has no end token.  Empty captions, full-length captions and a
        candidate equal to a reference are present.  Document frequencies are those of the 12 images (every pass scores all 12).
self_critical_train.npz
    the reference MODEL on the existing subgc_train golden inputs and weights (dropout 0, like that case) with the objective
    RewardCriterion()(outputs[:, :T].gather(2, seq.unsqueeze(2)).squeeze(2), seq, reward) + gpn_loss, where the model is teacher-forced on
    labels = [0, seq, 0] for a seeded `seq`, and reward = score(seq) - score(greedy) with score = w_cider * CIDEr + w_bleu * BLEU-4 of the
    reference's scorers against seeded references of the batch's three images.  Stored: the tokens, the references, the weights, the
    scores and rewards, the losses and the gradient of every live parameter under its own name.

    python tests/golden/make_golden_self_critical.py
"""
import contextlib
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (helpers only: ref_opt, build, enter_scratch, np_)

S, T = 3, 5
N_IMG, N_CAND, L, V = 12, 20, 10, 14
W_CIDER, W_BLEU = 1.0, 0.5


def array_to_str(row):
    """The upstream array_to_str: the ids as decimal strings, the end token included, nothing behind it."""
    out = []
    for w in row:
        out.append(str(int(w)))
        if int(w) == 0:
            break
    return " ".join(out)


def criterion_case(RewardCriterion):
    gen = torch.Generator().manual_seed(20261)
    inp = -torch.rand(S, T, generator=gen) * 6.0 - 0.01
    seq = torch.randint(1, 40, (S, T), generator=gen)
    seq[0, 3:] = 0                     # ends in mid-sentence: two masked-out steps
    seq[1] = 0                         # a row of all zeros: only its first step counts
    r_row = torch.tensor([-0.75, 0.0, 1.25]).view(S, 1).expand(S, T).contiguous()          # negative / zero / positive, constant along t
    r_tok = torch.randn(S, T, generator=gen)
    r_tok[2, 1] = 0.0
    gpn = torch.rand(S, generator=gen) + 0.1
    out = dict(input=MG.np_(inp), seq=seq.numpy(), reward_row=MG.np_(r_row), reward_tok=MG.np_(r_tok), gpn_loss=MG.np_(gpn))
    keys = []
    for rname, r in (("row", r_row), ("tok", r_tok)):
        for with_gpn in (False, True):
            x = inp.clone().requires_grad_(True)
            g = gpn.clone().requires_grad_(True) if with_gpn else None
            loss = RewardCriterion()(x, seq, r, g)
            loss.backward()
            key = f"{rname}_{'gpn' if with_gpn else 'plain'}"
            keys.append(key)
            out[f"loss_{key}"], out[f"dinput_{key}"] = MG.np_(loss), MG.np_(x.grad)
            if with_gpn:
                out[f"dgpn_{key}"] = MG.np_(g.grad)
    return out, keys


def scorers():
    sys.path[:0] = [os.path.join(MG.REF, "misc", "coco-caption"), MG.REF]
    from pycocoevalcap.bleu.bleu import Bleu
    from pycocoevalcap.cider.cider import Cider
    return Bleu, Cider


def score_rows(Bleu, Cider, refs, cand, cand_img):
    """Every candidate row scored by the reference's scorers against ITS image, with the document frequencies of ALL images: one pass per
    row, in which the other images answer with their first reference.  -> (bleu [rows, 4], cider [rows])."""
    n_img = len(refs)
    gts = {100 + j: [array_to_str(r) for r in refs[j]] for j in range(n_img)}
    bleu, cider = np.zeros((len(cand), 4)), np.zeros(len(cand))
    for r, row in enumerate(cand):
        j = int(cand_img[r])
        res = {100 + i: [gts[100 + i][0]] for i in range(n_img)}
        res[100 + j] = [array_to_str(row)]
        with contextlib.redirect_stdout(io.StringIO()):
            b = Bleu(4).compute_score(gts, res)[1]
            c = Cider().compute_score(gts, res)[1]
        bleu[r] = [b[k][j] for k in range(4)]
        cider[r] = np.asarray(c)[j]
    return bleu, cider


def random_caption(rng, length, width, vocab):
    row = np.zeros(width, np.int64)
    row[:length] = rng.integers(1, vocab + 1, length)
    return row


def score_case(Bleu, Cider):
    rng = np.random.default_rng(20262)
    refs = []
    for j in range(N_IMG):
        n = 1 + j % 5
        caps = [random_caption(rng, int(rng.integers(2, L + 1)), L, V) for _ in range(n)]
        refs.append(np.stack(caps))
    refs[3][0] = 0                                                   # an empty reference caption
    refs[4][0] = rng.integers(1, V + 1, L)                           # a full-length one: no end token
    cand_img = rng.integers(0, N_IMG, N_CAND)
    cand_img[:3] = [3, 4, 5]
    cand = np.zeros((2 * N_CAND, L), np.int64)
    for r in range(2 * N_CAND):
        j = int(cand_img[r % N_CAND])
        base = refs[j][int(rng.integers(0, len(refs[j])))].copy()    # a reference of its image, perturbed: the scores are not all zero
        n = int((base > 0).sum())
        for _ in range(int(rng.integers(0, 4))):
            if n:
                base[int(rng.integers(0, n))] = rng.integers(1, V + 1)
        if rng.random() < 0.3 and n > 2:
            base[n - 1] = 0
        cand[r] = base
    cand[0] = 0                                                      # empty captions (sampled and greedy)
    cand[N_CAND + 7] = 0
    cand[1] = rng.integers(1, V + 1, L)                              # full-length captions
    cand[N_CAND + 1] = refs[4][0]                                    # ... one of them equal to the full-length reference
    cand[2] = refs[5][0]                                             # a candidate equal to a reference
    bleu, cider = score_rows(Bleu, Cider, refs, cand, np.concatenate([cand_img, cand_img]))
    cap_off = np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.int64)
    return dict(ref_rows=np.concatenate(refs), ref_cap_off=cap_off, cand=cand, cand_img=cand_img.astype(np.int64), bleu=bleu, cider=cider)


def write_npz(path, out):
    # an .npz like np.savez_compressed writes it, deflated at the highest level
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for k, v in out.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(v), allow_pickle=False)
            zf.writestr(k + ".npy", buf.getvalue())


def train_case(RewardCriterion, Bleu, Cider):
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
    b5, Tm, Vm, B = batch["labels"].size(0), batch["labels"].size(1) - 2, MG.TINY["vocab_size"], base["B"]
    rng = np.random.default_rng(20263)
    refs = [np.stack([random_caption(rng, int(rng.integers(3, Tm + 1)), Tm, Vm) for _ in range(2 + j)]) for j in range(B)]
    gt_indices = np.array([2, 0, 1], np.int64)                          # batch image i is reference image gt_indices[i]
    spi = b5 // B
    seq2 = np.zeros((2 * b5, Tm), np.int64)
    for r in range(2 * b5):
        j = int(gt_indices[(r % b5) // spi])
        row = refs[j][int(rng.integers(0, len(refs[j])))].copy()
        n = int((row > 0).sum())
        for _ in range(int(rng.integers(0, 6))):
            row[int(rng.integers(0, n))] = rng.integers(1, Vm + 1)
        if rng.random() < 0.4:
            row[int(rng.integers(1, n)):] = 0
        seq2[r] = row
    seq2[4] = 0                                                         # an empty sampled caption
    seq2[6] = rng.integers(1, Vm + 1, Tm)                               # a full-length one
    img_of_row = np.concatenate([gt_indices[np.arange(b5) // spi]] * 2)
    bleu, cider = score_rows(Bleu, Cider, refs, seq2, img_of_row)
    scores = W_CIDER * cider + W_BLEU * bleu[:, 3]
    reward = (scores[:b5] - scores[b5:]).astype(np.float32)
    seq = torch.from_numpy(seq2[:b5])
    labels = torch.zeros(b5, Tm + 2, dtype=torch.long)
    labels[:, 1:Tm + 1] = seq
    fed = {k: v.clone() for k, v in batch.items()}
    fed["labels"] = labels
    outputs, gpn_loss, score = model(*synthetic.forward_args(fed))
    rw = torch.from_numpy(reward).view(b5, 1).expand(b5, Tm)
    lang_loss = RewardCriterion()(outputs[:, :Tm].gather(2, seq.unsqueeze(2)).squeeze(2), seq, rw)
    loss = lang_loss + gpn_loss
    loss.backward()
    out = {"lang_loss": MG.np_(lang_loss), "gpn_loss": MG.np_(gpn_loss), "loss": MG.np_(loss)}
    out.update({k: MG.np_(p.grad) for k, p in model.named_parameters() if p.grad is not None})      # every other key is a parameter's name
    out.update({"sc.seq2": seq2, "sc.ref_rows": np.concatenate(refs), "sc.gt_indices": gt_indices,
                "sc.ref_cap_off": np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.int64),
                "sc.weights": np.array([W_CIDER, W_BLEU]), "sc.scores": scores, "sc.reward": reward, "sc.mean_reward": np.float64(reward.astype(np.float64).mean())})
    write_npz(os.path.join(HERE, "self_critical_train.npz"), out)


def main():
    assert os.path.isdir(MG.REF), "golden vectors can only be regenerated where the reference exists"
    MG.enter_scratch()
    from misc.utils import RewardCriterion
    Bleu, Cider = scorers()
    out, keys = criterion_case(RewardCriterion)
    out.update(score_case(Bleu, Cider))
    np.savez_compressed(os.path.join(HERE, "self_critical_case.npz"), **out)
    meta = dict(S=S, T=T, keys=keys, zero_row=1, full_row=2, n_img=N_IMG, n_cand=N_CAND, L=L, V=V, empty_cands=[0, N_CAND + 7],
                full_cands=[1, N_CAND + 1], equal_cands=[[2, 5, 0], [N_CAND + 1, 4, 0]], empty_ref=[3, 0], full_ref=[4, 0],
                source="misc/utils.py:89-109 (RewardCriterion), pycocoevalcap Cider / Bleu(4); fp32 / fp64, CPU")
    with open(os.path.join(HERE, "self_critical_meta.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    train_case(RewardCriterion, Bleu, Cider)


if __name__ == "__main__":
    main()
