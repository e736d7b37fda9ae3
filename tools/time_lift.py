"""time the lift of a BED file through a piece table (mxg_lift_prepare, mxg_lift_intervals, mxg_lift_bed):
    MXG_DEBUG_IO=1 python tools/time_lift.py [--contigs 20000] [--features 2000000] [--runs 3] [--dir DIR]
A synthetic run: --contigs contigs of 20 to 400 kbp, one in five cut in two with a trimmed stretch between the halves, every other
piece reversed, four pieces a scaffold with gaps between them; --features features of 100 to 5000 bases spread over the contigs, six
BED columns.  One handle: the index build, then per run the lookup alone (lift_intervals over the parsed features) and the whole
lift_bed.  The library prints the device times of every call (HIP events) and lift_bed's host parse, lift and format + write times on
stderr; the wall time of every call is printed here, and the wall time of the serial host route (tools/lift_check.cpp, built with
-O2) on the same input.  The first call of each pays its allocations."""
import argparse
import os
import random
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, ".")
from ntjoin_amd.engine import MxEngine  # noqa: E402

FWD, REV, GAP = 0, 1, 2


def make_table(n_contigs, rng):
    lengths = [rng.randint(20_000, 400_000) for _ in range(n_contigs)]
    pieces = []
    for r, L in enumerate(lengths):
        if r % 5 == 0:
            cut = rng.randint(L // 4, 3 * L // 4)
            pieces += [(r, 0, cut, rng.choice((FWD, REV))), (r, min(L - 1, cut + rng.randint(0, 300)), L, rng.choice((FWD, REV)))]
        else:
            pieces.append((r, 0, L, FWD if r % 2 else REV))
    rng.shuffle(pieces)
    rows, first = [], [0]
    for i in range(0, len(pieces), 4):
        for j, p in enumerate(pieces[i:i + 4]):
            if j:
                rows.append((0, 0, rng.randint(20, 2000), GAP))
            rows.append(p)
        first.append(len(rows))
    return lengths, np.asarray(rows, dtype=np.uint32), np.asarray(first, dtype=np.uint64)


def write_bed(path, lengths, n_features, rng):
    rec, start, end = [], [], []
    with open(path, "w") as fh:
        for i in range(n_features):
            r = rng.randrange(len(lengths))
            n = rng.randint(100, 5000)
            a = rng.randrange(max(1, lengths[r] - n))
            b = min(lengths[r], a + n)
            fh.write(f"ctg{r}\t{a}\t{b}\tf{i}\t{i % 1000}\t{'+-'[i & 1]}\n")
            rec.append(r), start.append(a), end.append(b)
    return (np.asarray(x, dtype=np.uint32) for x in (rec, start, end))


def wall(fn):
    t0 = time.perf_counter()
    res = fn()
    return time.perf_counter() - t0, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=20000)
    ap.add_argument("--features", type=int, default=2_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the input and output files go (default: a temporary directory)")
    ap.add_argument("--no_host", action="store_true", help="leave the serial host route out")
    a = ap.parse_args()
    rng = random.Random(1)
    d = a.dir or tempfile.mkdtemp(prefix="time_lift_")
    os.makedirs(d, exist_ok=True)
    lengths, rows, first = make_table(a.contigs, rng)
    bed = os.path.join(d, "features.bed")
    rec, start, end = write_bed(bed, lengths, a.features, rng)
    src = [f"ctg{r}" for r in range(a.contigs)]
    dst = [f"ntJoin{r}" for r in range(len(first) - 1)]
    print(f"{a.contigs} contigs, {len(rows)} pieces in {len(dst)} scaffolds, {a.features} features, BED of {os.path.getsize(bed)} bytes", flush=True)
    with MxEngine(k=32, w=1000) as eng:
        for run in range(a.runs):
            s_prep, _ = wall(lambda: eng.lift_prepare(rows, first, lengths))
            s_look, res = wall(lambda: eng.lift_intervals(rec, start, end))
            s_bed, st = wall(lambda: eng.lift_bed(bed, src, dst, os.path.join(d, "gpu.lifted.bed"), os.path.join(d, "gpu.unlifted.bed")))
            print(f"run {run + 1}: lift_prepare {s_prep * 1e3:.2f} ms wall, lift_intervals {s_look * 1e3:.2f} ms wall ({len(res[2])} parts, "
                  f"with the copies to the host and into numpy), lift_bed {s_bed * 1e3:.2f} ms wall ({st['parts']} parts, "
                  f"{st['lifted_bytes']} + {st['unlifted_bytes']} bytes)", flush=True)
    if a.no_host:
        return 0
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    exe = os.path.join(d, "lift_check")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-I", "include", "-I", "ntjoin_amd/csrc", "tools/lift_check.cpp", "-o", exe])
    with open(os.path.join(d, "table.txt"), "w") as fh:
        words = [len(lengths)] + lengths + [len(first) - 1]
        for r in range(len(first) - 1):
            rec_rows = rows[int(first[r]):int(first[r + 1])]
            words.append(len(rec_rows))
            words.extend(rec_rows.reshape(-1).tolist())
        fh.write(" ".join(map(str, words)) + "\n")
    with open(os.path.join(d, "names.txt"), "w") as fh:
        fh.write("".join(n + "\n" for n in src + dst))
    for run in range(a.runs):
        s_host, _ = wall(lambda: subprocess.check_call([exe, "bed", os.path.join(d, "table.txt"), os.path.join(d, "names.txt"), bed,
                                                        os.path.join(d, "host.lifted.bed"), os.path.join(d, "host.unlifted.bed")],
                                                       stdout=subprocess.DEVNULL))
        print(f"run {run + 1}: lift_check bed (serial host route: reads the table, sorts, parses, lifts, writes) {s_host * 1e3:.2f} ms wall", flush=True)
    same = all(open(os.path.join(d, "gpu." + n), "rb").read() == open(os.path.join(d, "host." + n), "rb").read() for n in ("lifted.bed", "unlifted.bed"))
    print("the two routes' files are " + ("the same" if same else "DIFFERENT"), flush=True)
    if not a.dir:
        shutil.rmtree(d, ignore_errors=True)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
