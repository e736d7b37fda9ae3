#!/usr/bin/env python3
"""Times mxg_write_scaffolds: best of 3 calls on a synthetic target of --mbp Mbp (lines of 80, a few runs of N)
with paths of three nodes that cover most of it, overlap stage on; seconds and GB of output text per second for the whole call
(device, copies to the host, writing the three files), and for scale the Python restatement's rate on a slice of the same input.

  python tools/time_scaffolds.py [--mbp 200 1000] [--cpu-mbp 50] [--dir /dev/shm]

The two kernels' own times: run it under `rocprofv3 --kernel-trace --stats -- python tools/time_scaffolds.py --mbp 1000 --cpu-mbp 0`
(a run of its own) and read k_scaf_ends / k_scaf_emit; the emit kernel moves, per output byte, one byte read (plus the line ends it
squeezes out, 1/80 here) and one byte written."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ntjoin_amd import synth  # noqa: E402
from ntjoin_amd.engine import MxEngine  # noqa: E402


def make_input(mbp, fasta, n_rec=4, step=10_000, length=9_900, per_path=3):
    rec_len = mbp * 1_000_000 // n_rec // 80 * 80
    rng = np.random.default_rng(7)
    texts = []
    with open(fasta, "wb") as fh:
        for r in range(n_rec):
            text = np.frombuffer(synth.to_ascii(synth.make_reference(40 + r, rec_len)[0]), dtype=np.uint8).copy()
            for at in rng.integers(0, rec_len - 20_000, size=max(1, rec_len // 2_000_000)).tolist():
                text[at:at + int(rng.choice([10, 500, 9000]))] = ord("N")
            texts.append(text)
            fh.write(f">chr{r}\n".encode("ascii"))
            body = np.full((rec_len // 80, 81), ord("\n"), dtype=np.uint8)
            body[:, :80] = text.reshape(-1, 80)
            fh.write(body.tobytes())
    per_rec = (rec_len - length) // step // per_path * per_path
    nodes = np.zeros(n_rec * per_rec, dtype=MxEngine.SCAFFOLD_NODE)
    for r in range(n_rec):
        part = nodes[r * per_rec:(r + 1) * per_rec]
        part["record"] = r
        part["start"] = np.arange(per_rec, dtype=np.uint32) * step
    nodes["end"] = nodes["start"] + length
    nodes["gap_size"] = 20
    nodes["gap_size"][per_path - 1::per_path] = 0
    nodes["reverse"] = np.arange(len(nodes)) % 7 == 0
    nodes["end_adjust"] = np.where(np.arange(len(nodes)) % 5 == 1, length - 40, 0)
    first = np.arange(len(nodes) // per_path + 1, dtype=np.uint64) * per_path
    return texts, nodes, first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=int, nargs="+", default=[200, 1000])
    ap.add_argument("--cpu-mbp", type=int, default=50)
    ap.add_argument("--dir", default=None, help="where the FASTA and the outputs go (default: the system's temporary directory)")
    args = ap.parse_args()
    for mbp in args.mbp:
        with tempfile.TemporaryDirectory(dir=args.dir) as td:
            fasta = os.path.join(td, "t.fa")
            texts, nodes, first = make_input(mbp, fasta)
            names = [os.path.join(td, f) for f in ("a.fa", "u.fa", "u.bed")]
            with MxEngine(k=32, w=1000) as eng:
                a = eng.add_fasta("t", 1.0, fasta)
                call = lambda: eng.write_scaffolds(a, nodes, first, overlap_gap=20, assigned=names[0], unassigned=names[1], bed=names[2])  # noqa: E731
                res = call()  # (the first call allocates)
                times = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    call()
                    times.append(time.perf_counter() - t0)
                best = min(times)
            out = os.path.getsize(names[0]) + os.path.getsize(names[1])
            stripped = int((res["lead_strip"] > 0).sum() + (res["tail_strip"] > 0).sum())
            print(f"{mbp} Mbp, {len(first) - 1} paths ({stripped} stripped ends): {out / 1e9:.3f} GB of text out, best of 3 = {best:.3f} s, "
                  f"{out / best / 1e9:.2f} GB/s")
            if args.cpu_mbp:
                from tests import _scaffold_restatement as rs
                n_bases = min(args.cpu_mbp * 1_000_000, len(texts[0]))
                seq = texts[0][:n_bases].tobytes().decode("ascii")
                sub = [nd for nd in nodes[:int(first[-1])] if nd["record"] == 0 and nd["end"] <= n_bases]
                sub = sub[:len(sub) // 3 * 3]
                paths = [[("chr0", "-" if nd["reverse"] else "+", int(nd["start"]), int(nd["end"]), int(nd["gap_size"]),
                           int(nd["start_adjust"]), int(nd["end_adjust"])) for nd in sub[i:i + 3]] for i in range(0, len(sub), 3)]
                t0 = time.perf_counter()
                text, _, _ = rs.scaffolds(paths, {"chr0": seq}, 20)
                _bed, un, _n = rs.unassigned([("chr0", seq)], paths)
                dt = time.perf_counter() - t0
                print(f"  restatement on the CPU (strings in memory, nothing read or written): {(len(text) + len(un)) / dt / 1e9:.2f} GB/s")


if __name__ == "__main__":
    main()
