#!/usr/bin/env python3
"""Times mxg_overlap_cuts: best of 5 calls for N junctions with overlaps of 500 bases on a random assembly,
and for scale the Python restatement's junctions per second on a sample of the same input.

  python tools/time_overlap.py [--junctions 100000 1000000] [--cpu-sample 200]

The split between the two kernels: run it under `rocprofv3 --kernel-trace --stats -- python tools/time_overlap.py --junctions 100000`
(a run of its own) and read ov_node / ov_junction."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ntjoin_amd import synth  # noqa: E402
from ntjoin_amd.engine import MxEngine  # noqa: E402


def make_input(n_junctions, step=500, length=1000, per_path=20):
    n_paths = (n_junctions + per_path - 2) // (per_path - 1)
    n_nodes = n_paths * per_path
    nodes = np.zeros(n_nodes, dtype=MxEngine.OVERLAP_NODE)
    nodes["start"] = np.arange(n_nodes, dtype=np.uint32) * step
    nodes["end"] = nodes["start"] + length
    nodes["raw_gap"] = -(length - step)
    nodes["raw_gap"][per_path - 1::per_path] = 0
    first = np.arange(n_paths + 1, dtype=np.uint64) * per_path
    return nodes, first, n_paths * (per_path - 1), step * n_nodes + length


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--junctions", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--cpu-sample", type=int, default=200)
    ap.add_argument("-k", type=int, default=15)
    ap.add_argument("-w", type=int, default=10)
    args = ap.parse_args()
    for n in args.junctions:
        nodes, first, junctions, bases = make_input(n)
        text = synth.to_ascii(synth.make_reference(3, bases)[0])
        with MxEngine(k=32, w=1000) as eng:
            a = eng.add_records("t", 1.0, [("g", text)])
            eng.overlap_cuts(a, nodes, first, k=args.k, w=args.w)  # allocations
            best = None
            for _ in range(5):
                t0 = time.perf_counter()
                res = eng.overlap_cuts(a, nodes, first, k=args.k, w=args.w)
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
        print(f"{junctions} junctions ({bases / 1e6:.1f} Mbp, {int(res['cut_found'].sum())} cuts): best of 5 = {best * 1e3:.2f} ms, "
              f"{junctions / best / 1e6:.2f} M junctions/s")
        if args.cpu_sample:
            from tests import _oracle, _overlap_restatement as rs
            orc = _oracle.load()
            per = int(first[1])
            m = max(1, args.cpu_sample // (per - 1))
            paths = [[("g", "+", int(nd["start"]), int(nd["end"]), int(nd["raw_gap"])) for nd in nodes[p * per:(p + 1) * per]]
                     for p in range(m)]
            s = text.decode("ascii")[:int(nodes["end"][m * per - 1])]
            t0 = time.perf_counter()
            rs.cuts(paths, {"g": s}, args.k, args.w, lambda t, k, w: [(h, p) for h, p, _f, _m in orc.sketch(t, k, w)])
            dt = time.perf_counter() - t0
            print(f"  restatement on the CPU: {m * (per - 1) / dt:.0f} junctions/s")


if __name__ == "__main__":
    main()
