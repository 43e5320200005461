#!/usr/bin/env python3
"""The proposal chain (subgc.proposals.ProposalSampler.sample: seed draw, expansion, duplicate removal, the one host read, the kept
rows and the loader items) beside the decode of the same images, at bench.py's Sub_GC_Kar model.

    python tools/proposals_bench.py [--out profiles/r26_proposals_bench.txt] [--rounds 5] [--inner 3]

Shapes: 256 images x n = 100 draws (the Karpathy test setting: NMS 0.75, at most 10 captions per image, greedy) and 4 images x
n = 1000 draws (the MRNN setting of test.sh: NMS 0.55, at most 1000, top-k sampling k = 3, T = 0.6).  36 nodes + the dummy node,
40 relations per image (rel_num 65), 2048-d region features, 1599 object classes, 21 predicate classes, seeds (1, 3).
Method: both legs warmed up, then `rounds` rounds in which the legs alternate; a leg's round value is the median of `inner` calls,
host clock around the call + synchronise; reported: the median of the round medians and their spread (max - min).  The host time
of the item dictionaries (`control_input._items`: views and Python dicts, no launch) is clocked inside the chain's calls."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sub-gc_amd"), ROOT]
import numpy as np  # noqa: E402

OBJ_NUM, REL_NUM, D, C, PD, N_REL = 37, 65, 2048, 1599, 21, 40


def make_raw(images, seed, dev):
    import torch
    rng = np.random.default_rng(seed)
    n = OBJ_NUM - 1
    t = lambda x, dt=None: torch.from_numpy(np.ascontiguousarray(x)).to(device=dev, dtype=dt)  # noqa: E731
    return dict(object_fmap=t(np.abs(rng.standard_normal((images, n, D), dtype=np.float32))), object_dist=t(rng.random((images, n, C), dtype=np.float32)),
                rel_ind=t(rng.integers(0, n, size=(images * N_REL, 2)), torch.int64), pred_dist=t(rng.random((images * N_REL, PD), dtype=np.float32)),
                rel_off=t(np.arange(images + 1) * N_REL, torch.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_proposals_bench.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    a = ap.parse_args()

    import torch
    import bench
    import subgc.models as models
    from subgc import control_input as CI
    from subgc import proposals as P
    assert torch.cuda.is_available(), "proposals_bench needs the MI355X"
    dev = torch.device("cuda:0")
    spent = [0.0]
    real_items = CI._items

    def clocked_items(*args, **kw):
        t0 = time.perf_counter()
        out = real_items(*args, **kw)
        spent[0] += time.perf_counter() - t0
        return out
    P._items = clocked_items

    lines = ["proposals bench: raw scene graph -> seed draw -> expansion -> duplicate removal -> loader items, beside the decode of those items; "
             f"Sub_GC_Kar model sizes, {OBJ_NUM - 1} nodes, {N_REL} relations, D = {D}, C = {C}, seeds (1, 3); median of {a.rounds} round medians "
             f"({a.inner} calls a round, legs alternating), spread = max - min of the round medians"]
    shapes = [("256 images x n = 100, Karpathy decode (NMS 0.75, <= 10 captions, greedy)", 256, 100, dict(test_LSTM=1, gpn_nms_thres=0.75, gpn_max_subg=10)),
              ("4 images x n = 1000, MRNN decode (NMS 0.55, <= 1000 captions, top-k sampling)", 4, 1000, dict(bench.MRNN))]
    for title, images, n, mopt in shapes:
        torch.manual_seed(0)
        m = models.setup(argparse.Namespace(**dict(bench.KAR, **mopt))).to(dev).eval()
        sopt = dict(sample_max=1, beam_size=1)
        raw = make_raw(images, 100, dev)
        sampler = P.ProposalSampler(n, (1, 3), 2019, OBJ_NUM, REL_NUM)
        group = max(1, min(256, 8192 // int(mopt["gpn_max_subg"])))                              # caption_images' decode batch

        def chain():
            spent[0] = 0.0
            t0 = time.perf_counter()
            got = sampler.sample(raw)
            torch.cuda.synchronize()
            return got, 1e3 * (time.perf_counter() - t0), 1e3 * spent[0]

        def decode(items):
            t0 = time.perf_counter()
            with torch.no_grad():
                res = [r for i in range(0, len(items), group) for r in m.sample_images(items[i:i + group], opt=sopt)]
            torch.cuda.synchronize()
            return res, 1e3 * (time.perf_counter() - t0)

        for _ in range(2):
            got, _, _ = chain()
            res, _ = decode(got.items)
        r_chain, r_items, r_dec = [], [], []
        for _ in range(a.rounds):
            c, it, d = [], [], []
            for _ in range(a.inner):
                got, tc, ti = chain()
                _, td = decode(got.items)
                c.append(tc); it.append(ti); d.append(td)
            r_chain.append(statistics.median(c)); r_items.append(statistics.median(it)); r_dec.append(statistics.median(d))
        q = lambda x: f"{statistics.median(x):9.3f} ms (spread {max(x) - min(x):.3f})"  # noqa: E731
        kept, caps = got.table["kept"], sum(int(r[0].size(0)) for r in res)
        lines += [f"  {title}",
                  f"    kept candidates per image after duplicate removal: mean {kept.mean():.1f} (min {kept.min()}, max {kept.max()}) of {n}; "
                  f"captions decoded: {caps}",
                  f"    proposal chain, wall + synchronise:          {q(r_chain)}",
                  f"      of which the item dictionaries (host):     {q(r_items)}",
                  f"    decode of the same items (sample_images):    {q(r_dec)}",
                  f"    chain / decode (medians): {statistics.median(r_chain) / statistics.median(r_dec):.4f}"]
        del m, raw, got, res
        torch.cuda.empty_cache()
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
