#!/usr/bin/env python
"""Run the host transliteration of control_input.hip (tools/sct_host_check.cpp) on the loader fixture under AddressSanitizer and
UndefinedBehaviorSanitizer, on the CPU, and compare what it writes with the reference loader's arrays (tests/golden/sct_loader_case.npz).

    python tools/sct_host_check.py            # CXX=g++ by default

A stand-alone program with its own main(): nothing is loaded into python and no GPU is involved.  The batches are the GPU test's: the
four obj_num-37 greedy images in one batch (classes widened to one width with zero columns), the obj_num-65 image, the two gt images."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "sub-gc_amd")]


def main():
    import sct_loader_golden as G
    from subgc import control_input as CI
    meta, arr = G.load()
    tmp = tempfile.mkdtemp(prefix="sct_host_check_")
    exe = os.path.join(tmp, "sct_host_check")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "sct_host_check.cpp"), "-o", exe], check=True)
    checked = 0
    for tags in (("g0", "g1", "g2", "g4"), ("g3",), ("t0", "t1")):
        info = [meta["images"][t] for t in tags]
        gt = info[0]["mode"] == "gt"
        obj_num, rel_num, n_obj = info[0]["obj_num"], info[0]["rel_num"], info[0]["obj_num"] - 1
        C = max(arr[f"{t}_object_dist"].shape[1] for t in tags)
        dist = np.stack([np.pad(arr[f"{t}_object_dist"], ((0, 0), (0, C - arr[f"{t}_object_dist"].shape[1]))) for t in tags]).astype(np.float32)
        sets = np.concatenate([arr[f"{t}_sets"] for t in tags]).astype(np.float32)
        set_off = np.cumsum([0] + [arr[f"{t}_sets"].shape[0] for t in tags]).astype(np.int64)
        rels = [arr[f"{t}_rel_ind"].reshape(-1, 2).astype(np.int64) for t in tags]
        rel_off = np.cumsum([0] + [r.shape[0] for r in rels]).astype(np.int64)
        seed = np.concatenate([arr[f"{t}_seed"] for t in tags]).astype(np.int64) if gt else np.zeros(0, np.int64)
        seed_off = np.cumsum(np.concatenate([[0]] + [np.diff(arr[f"{t}_seed_off"]) for t in tags])).astype(np.int64) if gt else np.zeros(0, np.int64)
        B, n_sets, R = len(tags), sets.shape[0], sets.shape[1]
        head = np.array([B, n_obj, C, n_sets, R, obj_num, rel_num, int(rel_off[-1]), seed.size, int(gt)], np.int32)
        parts = [head, np.stack([arr[f"{t}_boxes"] for t in tags]).astype(np.float32), np.array([i["wh"] for i in info], np.float32), sets, set_off, dist,
                 np.concatenate(rels), rel_off, seed, seed_off]
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            for p in parts:
                f.write(np.ascontiguousarray(p).tobytes())
        subprocess.run([exe, fin, fout], check=True)
        buf, pos, out = open(fout, "rb").read(), 0, {}
        for name, dt, shape in (("seed", np.uint64, (n_sets,)), ("idx", np.int32, (n_sets, R)), ("iou", np.float32, (n_sets, R)), ("status", np.int32, (n_sets,)),
                                ("cls", np.int32, (B, n_obj)), ("gpn_obj_ind", np.int64, (n_sets, obj_num)), ("att_masks", np.float32, (n_sets, obj_num)),
                                ("gpn_pool_mtx", np.float32, (n_sets, obj_num, obj_num)), ("gpn_pred_ind", np.int64, (n_sets, rel_num)),
                                ("gpn_nrel_ind", np.int64, (n_sets, rel_num, 2)), ("choice", np.int32, (n_sets,)), ("status2", np.int32, (n_sets,))):
            n = int(np.prod(shape)) * np.dtype(dt).itemsize
            out[name] = np.frombuffer(buf[pos:pos + n], dt).reshape(shape)
            pos += n
        assert pos == len(buf)
        for b, t in enumerate(tags):
            a, e = int(set_off[b]), int(set_off[b + 1])
            s, i, v, st = CI.restate_match(arr[f"{t}_boxes"], info[b]["wh"], arr[f"{t}_sets"])
            assert (out["seed"][a:e] == s).all() and (out["idx"][a:e] == i).all() and out["iou"][a:e].tobytes() == v.tobytes() and (out["status"][a:e] == st).all(), t
            bad = info[b].get("bad_sets", [])
            ok = [k for k in range(e - a) if k not in bad]
            want = G.expected(meta, arr, t)
            if gt:
                off = arr[f"{t}_seed_off"]
                ch, st2 = CI.restate_gt_lookup(s, st, [arr[f"{t}_seed"][off[j]:off[j + 1]] for j in range(5)], n_obj)
                assert (out["choice"][a:e] == ch).all() and (out["status2"][a:e] == st2).all(), t
            else:
                assert (out["cls"][b] == np.argmax(dist[b], 1)).all(), t
                for key in G.ROWS:
                    assert (out[key][a:e][ok] == want[key][0, 0]).all() and (out[key][a:e][ok] == want[key][4, 1]).all(), (t, key)
            checked += e - a
    print(f"sct_host_check: {checked} region sets, address + undefined-behaviour sanitizers clean, outputs equal the reference loader's")


if __name__ == "__main__":
    main()
