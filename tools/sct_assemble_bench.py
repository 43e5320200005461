#!/usr/bin/env python3
"""Batch assembly of the controllability run (subgc.control_input.assemble_sct_batch: subgc_sct_match + subgc_sct_extract_greedy + the
padding kernels, with the one status / match-table copy) next to the `sct` decode of the rows it builds, and the reference loader's CPU
time for the same items.

    python tools/sct_assemble_bench.py [--out profiles/r18_sct_assemble_bench.txt] [--reps 30] [--images 200]
    python tools/sct_assemble_bench.py --script-only [--images 200]              (no GPU; where the reference lies)

Shape: `images` images x 5 region sets (1000 sets at the default), 36 detection boxes / nodes + the dummy node, 40 relations per image
(rel_num 65), 2048-d region features, 1599 object classes, 21 predicate classes, up to 6 region rows per set: test.sh's controllability
run at the Karpathy model sizes.  Boxes are integer boxes on a grid; a region is a detection box moved by a few pixels.
Method: warmed up, then timed `reps` times; device time = HIP events around the launches alone (the matching and extraction launches,
and the whole chain with the padding kernels), wall = host clock around assemble_sct_batch with its host copy of the status and match
tables; median, min and max are reported.  The decode is timed in the same process, same box: host clock around sample_images(sct=1) over
the assembled items + synchronise.
--script-only drives the reference's own `dataloader_test_sct.py` `__getitem__` (imported from where the reference lies, `h5py` stubbed,
the object given the attributes the method reads) over the same items on this CPU and appends its time to the file."""
import argparse
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sub-gc_amd"), ROOT]
import numpy as np  # noqa: E402

REF = os.environ.get("SUBGC_REFERENCE", "/root/reference")
OBJ_NUM, REL_NUM, D, C, PD, R, SETS, N_REL, S, LQ = 37, 65, 2048, 1599, 21, 6, 5, 40, 5, 16


def make_case(images, seed):
    """-> per image {object_fmap, object_dist, pred_dist, rel_ind, boxes, sets [SETS, R, 5], wh}."""
    rng = np.random.default_rng(seed)
    out = []
    n = OBJ_NUM - 1
    for _ in range(images):
        boxes = np.zeros((n, 4), np.float32)
        for k in range(n):
            x, y, w, h = 70 * (k % 8), 70 * (k // 8), int(rng.integers(20, 61)), int(rng.integers(20, 61))
            boxes[k] = [x, y, x + w - 1, y + h - 1]
        sets = np.zeros((SETS, R, 5), np.float32)
        for i in range(SETS):
            for j in range(int(rng.integers(1, R + 1))):
                sets[i, j, :4] = boxes[int(rng.integers(0, n))] + rng.integers(-6, 7, size=4)
                sets[i, j, 4] = 1
        out.append(dict(object_fmap=rng.standard_normal((n, D)).astype(np.float32), object_dist=rng.random((n, C)).astype(np.float32),
                        pred_dist=rng.random((N_REL, PD)).astype(np.float32), rel_ind=rng.integers(0, n, size=(N_REL, 2)), boxes=boxes, sets=sets,
                        wh=(592, int(rng.integers(300, 593)))))
    return out


def script_time(images, seed):
    sys.modules.setdefault("h5py", types.ModuleType("h5py"))
    sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    import torch
    from dataloaders.dataloader_test_sct import DataLoader
    case = make_case(images, seed)
    dl = object.__new__(DataLoader)
    dl.info = {"images": [{"id": i} for i in range(images)]}
    dl.seq_per_img, dl.seq_length, dl.obj_num, dl.rel_num, dl.use_greedy_subg, dl.use_gt_subg = S, LQ, OBJ_NUM, REL_NUM, 1, 0
    dl.label_start_ix, dl.label_end_ix = np.arange(images) * S + 1, (np.arange(images) + 1) * S
    dl.h5_label_file = {"labels": np.ones((images * S, LQ), np.int64)}
    dl.trip_loader = types.SimpleNamespace(get=lambda key: case[int(key)])
    dl.sct_dict = {str(i): torch.from_numpy(im["sets"]) for i, im in enumerate(case)}
    dl.img_wh = {i: im["wh"] for i, im in enumerate(case)}
    dl.__getitem__(0)
    t0 = time.perf_counter()
    n_sets = sum(int(dl.__getitem__(i)[-1][0]) for i in range(images))
    t = time.perf_counter() - t0
    return (f"reference on this CPU: dataloader_test_sct.py __getitem__ (--use_greedy_subg) over the same {images} images / {n_sets} region sets, one "
            f"process: {t:.2f} s ({1e3 * t / images:.1f} ms per image, {1e3 * t / n_sets:.2f} ms per set), numpy {np.__version__}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_sct_assemble_bench.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--script-only", action="store_true", help="only time the reference's loader on the CPU (needs no GPU, needs the reference)")
    a = ap.parse_args()
    if a.script_only:
        assert os.path.isdir(REF), "--script-only needs the reference"
        line = script_time(a.images, 100)
        print(line)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        return

    import torch
    import bench
    import subgc.models as models
    from subgc import control_input as CI
    assert torch.cuda.is_available(), "sct_assemble_bench needs the MI355X (or --script-only)"
    dev = torch.device("cuda:0")
    q = lambda x: f"median {statistics.median(x):.3f} (min {min(x):.3f}, max {max(x):.3f})"  # noqa: E731
    case = make_case(a.images, 100)
    t = lambda x, dt=None: torch.from_numpy(np.ascontiguousarray(x)).to(device=dev, dtype=dt)
    raw = dict(object_fmap=t(np.stack([im["object_fmap"] for im in case])), object_dist=t(np.stack([im["object_dist"] for im in case])),
               rel_ind=t(np.concatenate([im["rel_ind"] for im in case]), torch.int64), pred_dist=t(np.concatenate([im["pred_dist"] for im in case])),
               rel_off=t(np.arange(a.images + 1) * N_REL, torch.int64), boxes=t(np.stack([im["boxes"] for im in case])))
    sets = t(np.concatenate([im["sets"] for im in case]))
    off = (np.arange(a.images + 1) * SETS).tolist()
    wh = [im["wh"] for im in case]
    d_off, d_wh = torch.tensor(off, dtype=torch.int64, device=dev), torch.tensor(wh, dtype=torch.float32, device=dev)
    n_sets = off[-1]

    def kernels():
        seed, idx, iou, status = CI.match_regions(raw["boxes"], d_wh, sets, d_off)
        return CI.extract_greedy(raw["object_dist"], raw["rel_ind"], raw["rel_off"], d_off, seed, status, OBJ_NUM, REL_NUM)

    def chain():
        kernels()
        CI._graph_part(raw, OBJ_NUM, REL_NUM, None, S)

    for _ in range(3):
        items, table = CI.assemble_sct_batch(raw, sets, off, wh, OBJ_NUM, REL_NUM)
    ev_k, ev_c, wall = [], [], []
    for _ in range(a.reps):
        for fn, into in ((kernels, ev_k), (chain, ev_c)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            into.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        items, table = CI.assemble_sct_batch(raw, sets, off, wh, OBJ_NUM, REL_NUM)
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
    torch.manual_seed(0)
    m = models.setup(argparse.Namespace(**dict(bench.KAR, test_LSTM=1, sct=1))).to(dev).eval()
    sopt = dict(sample_max=1, beam_size=1, sct=1)
    dec = []
    with torch.no_grad():
        for _ in range(2):
            res = m.sample_images(items, opt=sopt)
        torch.cuda.synchronize()
        assert sum(r[2].size(0) // 2 for r in res) == n_sets
        for _ in range(max(5, a.reps // 4)):
            t0 = time.perf_counter()
            m.sample_images(items, opt=sopt)
            torch.cuda.synchronize()
            dec.append(1e3 * (time.perf_counter() - t0))
    nodes = float(torch.stack([it["att_masks"][0, 0].sum(-1) for it in items]).mean())
    lines = [f"sct assemble bench: region sets -> matched boxes -> greedy sub-graph rows -> loader items; {a.images} images x {SETS} region sets "
             f"({n_sets} sets, up to {R} regions each), {OBJ_NUM - 1} boxes, {N_REL} relations, D = {D}, C = {C}; {nodes:.1f} nodes kept per set on average, "
             f"{int((table['idx'] >= 0).sum())} matched regions",
             f"    subgc_sct_match + subgc_sct_extract_greedy, device ms (events, {a.reps} runs):      {q(ev_k)}",
             f"    the whole launch chain with the padding kernels, device ms (events, {a.reps} runs): {q(ev_c)}",
             f"    assemble_sct_batch: checks + launches + host copy of status / match table, wall ms: {q(wall)}",
             f"    decode of the assembled items (sample_images with sct=1, wall ms, {len(dec)} runs):      {q(dec)}",
             f"    assembly / decode (medians): device {statistics.median(ev_c) / statistics.median(dec):.5f}, wall "
             f"{statistics.median(wall) / statistics.median(dec):.4f}"]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
