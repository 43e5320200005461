#!/usr/bin/env python
"""Write the beam-attention fixture by RUNNING THE REFERENCE's beam search and then DRIVING ITS MODEL along every winning beam with
`get_logprobs_state(..., return_att=True)`, where the reference lies (never copied): beam_att_case.npz + beam_att_meta.json.  Data only:
the winning tokens, their lengths, the per-word attention rows, their arg-max and the gap between the two largest weights of every row.

    python tests/golden/make_golden_beam_att.py

The reference cannot ground a beam decode (misc/eval_utils.py:45 asserts beam_size == 1; `_sample_sentences`, AttModel.py:179-234, never
asks for `return_att`), so the yardstick is its own step function along the beam's winning tokens: per kept sub-graph, from
`init_hidden(1)`, step w is fed word w - 1 (<bos> at 0) and its attention row belongs to word w; a beam of length `len` (the end token
counted; T for a beam cut at the last step) has `len` rows.  The prepared features are the ones the beam search itself used (the output
of `_prepare_feature` is recorded during the search call).

Three configurations on inputs and weights that are already committed (make_golden.py): sGPN at beam 2 (subgc_beam2_wu), Full-GC at beam 3
(fullgc_greedy's image, fullgc_train's weights) and diverse beam search, beam 4 in 2 groups (subgc_beam4_div).

The tests compare arg-max nodes on every word whose reference top-2 gap is at least GAP = 1e-3 (ten times the attention tolerance); the
share of skipped words is written to the meta file and the script FAILS when the reference alone exceeds CAP = 5 % in a configuration --
then another image set is the remedy, not a looser cap."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG                                               # noqa: E402
from subgc import synthetic                                            # noqa: E402

GAP, CAP = 1e-3, 0.05
CASES = [("sgpn_beam2", "subgc_beam2_wu", "subgc_beam", None),
         ("fullgc_beam3", "fullgc_greedy", "fullgc_train", dict(sample_max=1, beam_size=3)),
         ("div_beam4", "subgc_beam4_div", "subgc_beam", None)]


def load(name):
    with np.load(os.path.join(HERE, name + ".npz")) as z:
        return {k: z[k].copy() for k in z.files}


def main():
    assert os.path.isdir(MG.REF), "golden vectors can only be regenerated where the reference exists"
    MG.enter_scratch()
    from models.AttModel import TopDownModel
    with open(os.path.join(HERE, "meta.json")) as f:
        all_meta = json.load(f)
    arr, meta = {}, {"gap": GAP, "cap": CAP, "cases": {}}
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self                     # CaptionModel.py:135,171 move the chosen words with .cuda()
    try:
        for name, src, weights, sample_opt in CASES:
            m_src = all_meta[src]
            sample_opt = dict(m_src["sample_opt"]) if sample_opt is None else sample_opt
            opt = MG.ref_opt(**m_src["opt"])
            torch.manual_seed(3)
            model = TopDownModel(opt)
            model.load_state_dict({k: torch.from_numpy(v) for k, v in load(weights + "_weights").items()})
            model.eval()
            batch = {k: torch.from_numpy(v) for k, v in load(src + "_inputs").items()}
            held = {}
            prep = model._prepare_feature
            model._prepare_feature = lambda *a, **k: held.setdefault("p", prep(*a, **k))
            with torch.no_grad():
                ret = model(*synthetic.sample_args({k: v.clone() for k, v in batch.items()}), opt=dict(sample_opt), mode="sample")
            model._prepare_feature = prep
            seq, seqlp = ret[0].numpy().astype(np.int64), ret[1].numpy()
            if sample_opt == m_src["sample_opt"]:                        # the same search the committed beam golden holds
                assert np.array_equal(seq, load(src + "_out")["seq"]), name
            p_fc, p_att, pp_att, p_mask = held["p"]
            n, T = seq.shape
            N = p_att.size(1)
            att, lens = np.zeros((n, T, N), np.float32), np.zeros(n, np.int32)
            with torch.no_grad():
                for s in range(n):
                    state = model.init_hidden(1)
                    words = seq[s].tolist()
                    lens[s] = words.index(0) + 1 if 0 in words else T
                    for w in range(lens[s]):
                        it = torch.tensor([0 if w == 0 else words[w - 1]], dtype=torch.long)
                        logprobs, state, a = model.get_logprobs_state(it, p_fc[s:s + 1], p_att[s:s + 1], pp_att[s:s + 1], p_mask[s:s + 1], state,
                                                                      return_att=True)
                        att[s, w, :a.size(1)] = a[0].numpy()
                        assert abs(float(logprobs[0, words[w]]) - float(seqlp[s, w])) < 1e-4, (name, s, w)    # the search's own step
            live = np.arange(T)[None, :] < lens[:, None]
            top2 = np.sort(att, 2)[:, :, -2:]
            gap = np.where(live, top2[:, :, 1] - top2[:, :, 0], 0).astype(np.float32)
            amax = np.where(live, att.argmax(2), -1).astype(np.int32)
            share = float((gap[live] < GAP).mean())
            assert share <= CAP, (name, "the reference's own attention rows are too often undecided", share)
            arr[name + "_tokens"], arr[name + "_len"], arr[name + "_att"] = seq, lens, att
            arr[name + "_argmax"], arr[name + "_gap"] = amax, gap
            meta["cases"][name] = dict(inputs=src, weights=weights, sample_opt=sample_opt, rows=int(n), words=int(live.sum()),
                                       skipped_share=share, min_gap=float(gap[live].min()), lens=lens.tolist())
            print(name, "rows", n, "words", int(live.sum()), "skipped share", share, "lens", lens.tolist())
    finally:
        torch.Tensor.cuda = orig_cuda
    np.savez_compressed(os.path.join(HERE, "beam_att_case.npz"), **arr)
    with open(os.path.join(HERE, "beam_att_meta.json"), "w") as f:
        json.dump(meta, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote beam_att_case.npz (%d bytes)" % os.path.getsize(os.path.join(HERE, "beam_att_case.npz")))


if __name__ == "__main__":
    main()
