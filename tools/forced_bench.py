#!/usr/bin/env python3
"""Forced decode and GT-sentence grounding (subgc.forced, subgc.grounding_gt, eval_glue.ground_gt_images) next to the GREEDY decode of the
same rows, and the stand-alone token filing at V = 9488.

    python tools/forced_bench.py [--out profiles/r17_forced_bench.txt] [--reps 20] [--images 64]

Shape: 64 images x 5 reference captions of 6 .. 16 words (Tf = 17 columns), the Karpathy sub-graph model of bench.py (vocabulary 9487),
every caption decoded on one of the image's candidate sub-graphs (its first five), 36 boxes and <= 4 annotated objects per caption.
Method: warmed up twice, then timed `reps` times with the host clock around the call plus a synchronise; median, min and max.
  forced decode            forced.forced_decode(return_att=True): encode, read-outs, Tf steps with subgc_forced_pick, subgc_forced_finish
  forced + GT grounding    eval_glue.ground_gt_images: the above + arg-max, material, score and the one host copy
  greedy decode, same rows the same encode, read-outs and Tf steps with subgc_decode_pick (k = 0) in the place of subgc_forced_pick
  pick alone               HIP events around 200 launches of subgc_forced_pick / subgc_decode_pick on the rows' logits [rows, 9488]
Both loops stream the same weights for the same rows, so they are expected to cost the same; the figures say whether they do."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sub-gc_amd"), ROOT]
import numpy as np  # noqa: E402

N_BOX, N_CAP, SEQ = 36, 5, 16


def make_refs(n_images, vocab_size, seed):
    rng = np.random.default_rng(seed)
    anns, boxes = [], {}
    for i in range(n_images):
        xy = rng.random((N_BOX + 1, 2)) * 300
        b = np.concatenate([xy, xy + 10 + rng.random((N_BOX + 1, 2)) * 200], 1).astype(np.float32)
        boxes[1000 + i] = b
        caps = []
        for _ in range(N_CAP):
            n_tok = int(rng.integers(6, SEQ + 1))
            pos = sorted(int(x) for x in rng.permutation(n_tok)[:int(rng.integers(0, 5))])
            caps.append({"tokens": [f"w{int(rng.integers(1, vocab_size + 1))}" for _ in range(n_tok)], "process_idx": pos,
                         "process_clss": [f"c{int(rng.integers(1, 31))}" for _ in pos],
                         "process_bnd_box": [(b[int(rng.integers(N_BOX))].astype(np.float64) + (0 if rng.random() < 0.6 else 35)).tolist() for _ in pos]})
        anns.append({"image_id": 1000 + i, "captions": caps})
    return anns, boxes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_forced_bench.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--images", type=int, default=64)
    a = ap.parse_args()

    import torch
    import bench
    import subgc.models as models
    from subgc import eval_glue, forced, grounding, ops, synthetic
    from subgc import functions as F_
    from subgc import grounding_gt as GT
    assert torch.cuda.is_available(), "forced_bench needs the MI355X"
    dev = torch.device("cuda:0")
    I = a.images
    q = lambda x: f"median {statistics.median(x):.3f} (min {min(x):.3f}, max {max(x):.3f})"  # noqa: E731
    torch.manual_seed(0)
    m = models.setup(argparse.Namespace(**dict(bench.KAR, test_LSTM=1, gpn_nms_thres=0.75, gpn_max_subg=10))).to(dev).eval()
    V = m.vocab_size
    images = [{k: v.to(dev) for k, v in synthetic.make_test_batch(50, seed=700 + i).items()} for i in range(I)]
    anns, boxes = make_refs(I, V, 100)
    ids = [x["image_id"] for x in anns]
    vocab = {str(i): f"w{i}" for i in range(1, V + 1)}
    refs = grounding.GroundingReferences(anns, ids, {i: f"c{i}" for i in range(1, 31)}, {}, {}, vocab, {}, device=dev)
    rows = GT.GtCaptionRows(anns, ids, vocab, SEQ, 1)
    gt = {"scorer": GT.GtGroundingScorer(refs), "index": {k: refs.index[str(k)] for k in ids}, "rows": rows, "boxes": boxes, "img_wh": None}
    infos = [{"id": k} for k in ids]
    tokens = [rows[k] for k in ids]
    counts = [len(t) for t in tokens]
    n, Tf = sum(counts), SEQ + 1

    def greedy_same_rows():
        att, obj, pred, rel = ops.stack_first([[im[k] for im in images] for k in ("att_feats", "obj_dist", "pred_dist", "rel_ind")])
        N = att.size(1)
        X2 = m._encode(att, obj, pred, rel).reshape(I * N, m.GCN_dim).contiguous()
        rows_in = [(i, im["gpn_obj_ind"], im["att_masks"], im["gpn_pool_mtx"]) for i, im in enumerate(images)]
        fc, lens, idx, img = forced._candidate_rows(m, X2, N, rows_in, counts)
        P = m._decoder_params()
        pr = F_.Prepared(fc, X2, lens, idx, img, N, P, None, None, 1.0)
        st = F_.DecodeState(pr, P, N, True, xt_table=m.xt_gates_table(), fuse_lstm=True, snapshots=m.decode_snapshots(), W16=m.decode_w16())
        z = lambda *s, dt=torch.float32: ops.zero_(torch.empty(*s, device=dev, dtype=dt))  # noqa: E731
        seq, seqlp, it, unf, cnt, AL = z(n, Tf, dt=torch.long), z(n, Tf), z(n, dt=torch.long), z(n, dt=torch.int32), z(Tf, dt=torch.int32), z(Tf, n, N)
        for t in range(Tf):
            logits = st.step(it, AL[t], normalize=False)
            ops.decode_pick(logits, 0, 1.0, None, t, seq, seqlp, it, unf, cnt[t:t + 1], cnt[t - 1:t] if t else None, raw=True)
        return seq, st.logits

    def timed(fn):
        for _ in range(2):
            r = fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            t = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t))
        return ms, r

    t_forced, d = timed(lambda: forced.forced_decode(m, images, tokens, return_att=True))
    t_gt, out = timed(lambda: eval_glue.ground_gt_images(m, images, infos, gt, group=I))
    t_greedy, (gseq, logits) = timed(greedy_same_rows)
    s = GT.summarize([e["gt_grounding"] for e in out], refs)
    ll = np.concatenate([e["caption_ll"]["ll"] for e in out])
    ntok = np.concatenate([e["caption_ll"]["n_tok"] for e in out])

    # the pick alone, on the last step's logits
    tok = d["tokens"]
    seq, seqlp = torch.zeros(n, Tf, device=dev, dtype=torch.long), torch.zeros(n, Tf, device=dev)
    it, unf, flag = torch.zeros(n, device=dev, dtype=torch.long), torch.zeros(n, device=dev, dtype=torch.int32), torch.zeros(1, device=dev, dtype=torch.int32)

    def events(fn, launches=200):
        for _ in range(20):
            fn()
        out_ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            e1.synchronize()
            out_ms.append(1e3 * e0.elapsed_time(e1) / launches)
        return out_ms

    p_forced = events(lambda: forced.forced_pick(logits, tok, 0, seq, seqlp, it, unf, flag, None, raw=True))
    p_greedy = events(lambda: ops.decode_pick(logits, 0, 1.0, None, 0, seq, seqlp, it, unf, flag, None, raw=True))
    lines = [f"forced bench: {I} images x {N_CAP} captions = {n} rows, Tf = {Tf}, Karpathy sub-graph model (V = {logits.size(1)} logit columns), "
             f"{int(ntok.sum())} scored tokens, {sum(len(e['gt_grounding']['events']) for e in out)} annotated objects",
             f"    forced decode (return_att), wall ms ({a.reps} runs):            {q(t_forced)}",
             f"    forced decode + GT grounding + host copy, wall ms ({a.reps} runs): {q(t_gt)}",
             f"    greedy decode of the same rows, wall ms ({a.reps} runs):          {q(t_greedy)}",
             f"    forced / greedy (medians): {statistics.median(t_forced) / statistics.median(t_greedy):.3f};  grounding on top of the forced decode: "
             f"{statistics.median(t_gt) - statistics.median(t_forced):+.3f} ms",
             f"    pick alone on [{n}, {logits.size(1)}] logits, us per launch (events, 200 launches x {a.reps}): subgc_forced_pick {q(p_forced)}; "
             f"subgc_decode_pick (greedy) {q(p_greedy)}",
             f"    summary: grd_accu {s['grd_accu']:.4f} over {s['n_classes']} classes (a randomly initialised model); mean NLL {-ll.sum() / ntok.sum():.4f} "
             f"(ln V = {np.log(logits.size(1)):.4f})"]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
