#!/usr/bin/env python
"""Time the nearest-image search (subgc.neighbours: subgc_nn_dist_f64 + subgc_nn_select_f64) at the reference's sizes -- D = 2048,
k = 1000 (conf_cr.py:14,51), 256 queries (one decode batch) against 29 000 (Flickr30k) and 113 000 (COCO) training rows -- beside the
Sub_GC_Kar decode of the 256-image batch it would precede, and scipy's cdist + argsort on the CPU for the same queries.

    python tools/nn_search_bench.py [--out profiles/r22_nn_search_bench.txt] [--rounds 5] [--inner 5] [--no-cpu] [--check]

Protocol: every leg is warmed, then `rounds` rounds run the legs INTERLEAVED (leg 1, leg 2, ... per round), each leg `inner` times per
round; a leg's figure is the median of its round medians, its spread the largest minus the smallest round median.  Kernel legs are device
events around the enqueues (no host copy inside), the decode leg a host clock around sample_images ending in a synchronise.
The bound: the distance kernel issues 3 fp64 vector instructions per (query, train, column) -- subtract, multiply, add; the contract
forbids fusing them -- and a CU retires 64 fp64 lane-operations per clock (4 SIMDs x 16 lanes; the chip's 78.6 TFLOP/s fp64 vector
figure counts an FMA as two), so least time = 3 Q N D / (CUs x 64 x clock).  --check also compares the device's sqrt and distances
with the host's on the first workload (np.sqrt is correctly rounded)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sub-gc_amd")]
Q, D, K = 256, 2048, 1000
SIZES = (29000, 113000)


def features(n, seed):
    rng = np.random.default_rng(seed)
    return np.maximum(rng.standard_normal((n, D), dtype=np.float32), 0)          # non-negative, like ResNet pool features; float32 values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_nn_search_bench.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true", help="skip scipy's cdist + argsort on the CPU")
    ap.add_argument("--no-decode", action="store_true", help="skip the decode leg")
    ap.add_argument("--check", action="store_true", help="compare device distances / sqrt with the host's")
    ap.add_argument("--sizes", default=",".join(str(n) for n in SIZES))
    a = ap.parse_args()
    import torch
    from subgc import neighbours, ops
    assert torch.cuda.is_available(), "nn_search_bench needs the MI355X"
    dev = torch.device("cuda:0")
    prop = torch.cuda.get_device_properties(0)
    cus, clock = prop.multi_processor_count, float(getattr(prop, "clock_rate", 2400000)) * 1e3
    lines = [f"nearest-image search bench: {Q} queries, D = {D}, k = {K}; {prop.name}, {cus} CUs at {clock / 1e9:.2f} GHz",
             f"protocol: legs interleaved, {a.rounds} rounds x {a.inner} runs, figure = median of round medians, spread = max - min of round medians"]
    te = features(Q, 1)
    legs, notes = {}, {}
    for n in [int(x) for x in a.sizes.split(",")]:
        index = neighbours.ImageIndex(features(n, 2 + n), device=dev)
        q = index.queries(te)
        ws = torch.empty(Q, n, device=dev, dtype=torch.float64)
        idx = torch.empty(Q, K, device=dev, dtype=torch.int32)
        val = torch.empty(Q, K, device=dev, dtype=torch.float64)
        legs[f"N = {n}: search (both kernels)"] = ("ev", lambda index=index, q=q, idx=idx, val=val: index.search(q, K, idx=idx, dist=val))
        legs[f"N = {n}: subgc_nn_dist_f64"] = ("ev", lambda index=index, q=q, ws=ws: ops.nn_dist(q, index.d_features, ws))
        legs[f"N = {n}: subgc_nn_select_f64"] = ("ev", lambda ws=ws, n=n, idx=idx, val=val: ops.nn_select(ws, n, K, idx, val))
        notes[n] = 3.0 * Q * n * D / (cus * 64 * clock) * 1e3
        if a.check and n == int(a.sizes.split(",")[0]):
            ops.nn_dist(q, index.d_features, ws)
            rows = ws[:4].cpu().numpy()
            s = np.zeros((4, n))
            tr = index.features
            for d in range(D):
                t = te[:4, d, None].astype(np.float64) - tr[None, :, d]
                s = s + t * t
            lines.append(f"check: {4 * n} device distances (4 query rows, N = {n}) against the numpy restatement: "
                         f"{int((rows.view(np.uint64) != np.sqrt(s).view(np.uint64)).sum())} differ in any bit")
    if not a.no_decode:
        import bench
        import subgc.models as models
        from subgc import synthetic
        torch.manual_seed(0)
        m = models.setup(argparse.Namespace(**dict(bench.KAR, test_LSTM=1, gpn_nms_thres=0.75, gpn_max_subg=10))).to(dev).eval()
        images = [{k: v.to(dev) for k, v in synthetic.make_test_batch(50, seed=700 + i).items()} for i in range(Q)]
        legs["decode: Sub_GC_Kar sample_images, 256 images"] = ("wall", lambda: m.sample_images(images, opt=dict(sample_max=1, beam_size=1), batch_out={"skip_att": True}))

    def run(kind, fn):
        if kind == "wall":
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for kind, fn in legs.values():
        for _ in range(2):
            run(kind, fn)
    rounds = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name, (kind, fn) in legs.items():
            rounds[name].append(statistics.median(run(kind, fn) for _ in range(a.inner)))
    fig = {name: statistics.median(r) for name, r in rounds.items()}
    for name, r in rounds.items():
        lines.append(f"  {name:50s} {fig[name]:9.3f} ms   spread {max(r) - min(r):.3f} ms")
    for n, least in notes.items():
        got = fig[f"N = {n}: subgc_nn_dist_f64"]
        lines.append(f"  N = {n}: distance kernel against its instruction bound: least {least:.3f} ms (3 x {Q} x {n} x {D} lane-operations), "
                     f"measured {got:.3f} ms = {100 * least / got:.1f} % of the bound's rate; select = {100 * fig[f'N = {n}: subgc_nn_select_f64'] / fig[f'N = {n}: search (both kernels)']:.1f} % of the search")
    dec = fig.get("decode: Sub_GC_Kar sample_images, 256 images")
    if dec:
        n0 = int(a.sizes.split(",")[0])
        lines.append(f"  search (N = {n0}) / the decode it precedes: {fig[f'N = {n0}: search (both kernels)'] / dec:.4f}")
    if not a.no_cpu:
        try:
            from scipy.spatial import distance
            n0 = int(a.sizes.split(",")[0])
            tr = features(n0, 2 + n0).astype(np.float64)
            t = time.perf_counter()
            dm = distance.cdist(te.astype(np.float64), tr, "euclidean")
            t1 = time.perf_counter()
            np.argsort(dm, axis=1)[:, :K]
            t2 = time.perf_counter()
            lines.append(f"  scipy on this machine's CPU, {Q} x {n0}: cdist {t1 - t:.2f} s + argsort {t2 - t1:.2f} s (one run) = "
                         f"{1e3 * (t2 - t) / fig[f'N = {n0}: search (both kernels)']:.0f} x the device search")
        except ImportError:
            lines.append("  scipy is not installed here: the CPU time of cdist + argsort was not measured")
    lines.append("not measured here: the upload of the training matrix (one-time), the host copy of find_nn, multi-GPU, and -- unless a "
                 "counter run is recorded below -- which of LDS reads, occupancy or global loads limits the distance kernel")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
