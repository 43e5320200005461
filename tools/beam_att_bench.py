#!/usr/bin/env python3
"""Beam search with the attention of the winning beams (`return_att = 1` with `beam_size > 1`) next to the same search without it and next
to the only way to get the same result without it: the search followed by a teacher-forced decode along the winners.

    python tools/beam_att_bench.py [--out profiles/r19_beam_att_bench.txt] [--rounds 5] [--reps 3] [--images 256]

Shapes: the one-image calls of test.sh (Sub_GC_Kar: beam 2, NMS 0.75, <= 10 sub-graphs; Full-GC: beam 3, one row; both replayed as a
hipGraph) over 16 images, and one decode batch of `images` Sub_GC_Kar images at beam 2 (eager).  Models of bench.py, fp32, random weights.
Legs, interleaved inside every round so that drift hits all three alike:
  off        beam decode, attention off (what the parent commit does)
  on         beam decode, attention on: step buffers and ancestry inside the search, one gather behind the ranking
  two-pass   `off`, then a forced decode along the winning tokens with attention output on the SAME kept sub-graphs: encode, selection
             (or the full-graph row), T steps with subgc_forced_pick.  This is cheaper than `forced.forced_decode`, which decodes an
             image's candidates in input order and would carry every candidate the NMS dropped.
Method: two warm-up calls per leg, then per round `reps` timed calls per leg (host clock around the call plus a synchronise; the median of
the round).  Reported: the median over the rounds and the spread (max - min) of the round medians, the overhead of `on` over `off` and
the ratio two-pass / on."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sub-gc_amd"), ROOT]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_beam_att_bench.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--images", type=int, default=256)
    a = ap.parse_args()

    import torch
    import bench
    import subgc.models as models
    from subgc import forced, ops, synthetic
    from subgc import functions as F_
    from subgc.models import sampling
    assert torch.cuda.is_available(), "beam_att_bench needs the MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    test = dict(test_LSTM=1, gpn_nms_thres=0.75, gpn_max_subg=10)
    kar = models.setup(argparse.Namespace(**dict(bench.KAR, **test))).to(dev).eval()
    full = models.setup(argparse.Namespace(**dict(bench.FULLGC, compute_dtype="fp32", **test))).to(dev).eval()
    images = [{k: v.to(dev) for k, v in synthetic.make_test_batch(50, seed=900 + i).items()} for i in range(a.images)]

    def second_pass(m, ims, seqs):
        """Forced decode with attention along `seqs` (one [rows_i, T] CPU tensor per image) on the sub-graphs the decode itself kept."""
        att, obj, pred, rel = ops.stack_first([[im[k] for im in ims] for k in ("att_feats", "obj_dist", "pred_dist", "rel_ind")])
        I, N, _ = att.shape
        X2 = m._encode(att, obj, pred, rel).reshape(I * N, m.GCN_dim).contiguous()
        rows_in = [(i, im["gpn_obj_ind"], im["att_masks"], im["gpn_pool_mtx"]) for i, im in enumerate(ims)]
        w = (sampling.select_subgraphs(m, X2, N, rows_in) if m.gpn else sampling.full_graph_rows(m, X2, N, rows_in)).whole
        P = m._decoder_params()
        pr = F_.Prepared(w["fc"], X2, w["lens"], w["idx"], w["img"], N, P, None, None, 1.0)
        st = F_.DecodeState(pr, P, N, True, xt_table=m.xt_gates_table(), fuse_lstm=True, snapshots=m.decode_snapshots())
        tok = torch.cat(seqs)
        n, T = tok.shape
        tok = ops.upload(tok.numpy().ravel(), torch.int64, dev).view(n, T)
        z = lambda *s, dt=torch.float32: ops.zero_(torch.empty(*s, device=dev, dtype=dt))  # noqa: E731
        seq, seqlp, it, unf, cnt, AL = z(n, T, dt=torch.long), z(n, T), z(n, dt=torch.long), z(n, dt=torch.int32), z(T, dt=torch.int32), z(T, n, N)
        for t in range(T):
            logits = st.step(it, AL[t], normalize=False)
            forced.forced_pick(logits, tok, t, seq, seqlp, it, unf, cnt[t:t + 1], cnt[t - 1:t] if t else None, raw=True)
        return AL

    def one_image(m, beam, ims):
        off, on = dict(sample_max=1, beam_size=beam), dict(sample_max=1, beam_size=beam, return_att=1)

        def leg_off():
            return [m(*synthetic.sample_args(b), opt=off, mode="sample") for b in ims]

        def leg_on():
            return [m(*synthetic.sample_args(b), opt=on, mode="sample") for b in ims]

        def leg_two():
            return [second_pass(m, [b], [m(*synthetic.sample_args(b), opt=off, mode="sample")[0].cpu()]) for b in ims]
        return leg_off, leg_on, leg_two

    def batch(m, beam, ims):
        off, on = dict(sample_max=1, beam_size=beam), dict(sample_max=1, beam_size=beam, return_att=1)

        def leg_off():
            return m.sample_images(ims, opt=off)

        def leg_on():
            return m.sample_images(ims, opt=on, batch_out={"skip_att": True})

        def leg_two():
            return second_pass(m, ims, [r[0].cpu() for r in m.sample_images(ims, opt=off)])
        return leg_off, leg_on, leg_two

    def measure(legs, per):
        for fn in legs:
            fn(); fn()
        torch.cuda.synchronize()
        rounds = [[] for _ in legs]
        for _ in range(a.rounds):
            for k, fn in enumerate(legs):
                ms = []
                for _ in range(a.reps):
                    t = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    ms.append(1e3 * (time.perf_counter() - t) / per)
                rounds[k].append(statistics.median(ms))
        return [(statistics.median(r), max(r) - min(r)) for r in rounds]

    one = images[:16]
    shapes = [("Sub_GC_Kar, beam 2, one image per call (hipGraph), ms per image", one_image(kar, 2, one), len(one)),
              ("Full-GC, beam 3, one image per call (hipGraph), ms per image", one_image(full, 3, one), len(one)),
              (f"Sub_GC_Kar, beam 2, one decode batch of {len(images)} images (eager), ms per batch", batch(kar, 2, images), 1)]
    lines = [f"beam attention bench: {a.rounds} rounds x {a.reps} calls per leg, legs interleaved; median of the round medians (spread = max - min of them)"]
    for title, legs, per in shapes:
        (off, s_off), (on, s_on), (two, s_two) = measure(legs, per)
        lines += [f"{title}",
                  f"    off       {off:9.3f}  (spread {s_off:.3f})",
                  f"    on        {on:9.3f}  (spread {s_on:.3f})    on - off {on - off:+.3f} ms = {100 * (on - off) / off:+.2f} %",
                  f"    two-pass  {two:9.3f}  (spread {s_two:.3f})    two-pass / on {two / on:.3f}"]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
