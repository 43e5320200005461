#!/usr/bin/env python
"""Run the host transliteration of subgc_nn_select_f64 (tools/nn_host_check.cpp, over the kernel's own sub-gc_amd/csrc/nn_select_logic.h)
on every case of the nearest-image fixture under AddressSanitizer and UndefinedBehaviorSanitizer, on the CPU, and compare the lists it
writes with the contract's (subgc.neighbours.find_nn_restatement) and, under the tie rule, with the reference's.

    python tools/nn_host_check.py            # CXX=g++ by default

A stand-alone program with its own main(): nothing is loaded into python and no GPU is involved."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "sub-gc_amd")]


def main():
    import neighbours_golden as G
    meta, arr = G.load()
    tmp = tempfile.mkdtemp(prefix="nn_host_check_")
    exe = os.path.join(tmp, "nn_host_check")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "nn_host_check.cpp"), "-o", exe], check=True)
    checked = 0
    for name, c in sorted(meta["cases"].items()):
        d, ref = arr[name + "_cdist"], arr[name + "_lists"]
        Q, N = d.shape
        order = np.argsort(G.keys(d), axis=1, kind="stable")
        for k in c["ks"]:
            fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            with open(fin, "wb") as f:
                f.write(np.array([Q, N, k], np.int64).tobytes())
                f.write(np.ascontiguousarray(d).tobytes())
            subprocess.run([exe, fin, fout], check=True)
            buf = open(fout, "rb").read()
            idx = np.frombuffer(buf[:Q * k * 4], np.int32).reshape(Q, k)
            val = np.frombuffer(buf[Q * k * 4:], np.float64).reshape(Q, k)
            assert (idx == order[:, :k]).all(), (name, k)
            assert val.tobytes() == np.take_along_axis(d, order[:, :k], 1).tobytes(), (name, k)
            G.compare_lists(idx, ref, d, k)
            checked += Q * k
    print(f"nn_host_check: {checked} list positions over {len(meta['cases'])} cases, address + undefined-behaviour sanitizers clean, "
          "lists equal the contract's and, under the tie rule, the reference's")


if __name__ == "__main__":
    main()
