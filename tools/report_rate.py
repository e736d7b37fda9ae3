"""tools/report_rate.py -- the measurement of DESIGN.md 4l (run it on an MI355X; about a minute, 2 GB of scratch files under TMPDIR): one FASTA of >= 1 GB written with mxg_synth_write_fasta, N runs put in at a few per Mbp; device times
of mxg_assembly_report and of mxg_write_fai's pass over the text (HIP events inside the library, MXG_DEBUG_IO), median of 5 after one
warm-up, alternating; then mxg_write_scaffolds with and without MXG_SCAF_REPORT on the same paths (host clock around the call, which ends
in a synchronise)."""
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ["MXG_DEBUG_IO"] = "1"
from ntjoin_amd import capi, synth  # noqa: E402
from ntjoin_amd.engine import MxEngine  # noqa: E402

work = tempfile.mkdtemp(prefix="report_rate_")
fa = os.path.join(work, "measure_report.fa")
log = os.path.join(work, "stderr.log")
MBP = 1040
N_REC = 16
lib = capi.load()
lens = np.full(N_REC, MBP * 1_000_000 // N_REC, dtype=np.uint64)
segs, n_words, _ = synth.reference_segments(lens)
words = synth.fill_device(segs, n_words, 5).cpu().numpy().view(np.uint32)
rs, rl = np.ascontiguousarray(segs[:, 0]), np.ascontiguousarray(segs[:, 2])
t0 = time.perf_counter()
assert lib.mxg_synth_write_fasta(fa.encode(), words.ctypes.data, rs.ctypes.data, rl.ctypes.data, len(rl), b"c", 80, 16) == 0
del words
size = os.path.getsize(fa)
# N runs: 3 per Mbp, lengths from 1 to 50 000, one of 30 Mbp (a centromere); line ends stay what they are
rng = np.random.default_rng(7)
mm = np.memmap(fa, dtype=np.uint8, mode="r+")
n_runs = 0
CENTRO = size // 2 + 20_000_000  # inside record 8, which no path takes
for at in rng.integers(100, size - 31_000_000, size=3 * MBP).tolist() + [CENTRO]:
    n = 30_000_000 if at == CENTRO else int(rng.choice([1, 5, 9, 10, 50, 300, 5000, 50_000]))
    seg = mm[at:at + n]
    seg[(seg != 10) & (seg != 62)] = ord("N")   # (a header caught by a run keeps its '>' and its line end; its name changes, nothing else)
    n_runs += 1
mm.flush()
del mm
print(f"fasta: {size} bytes, {N_REC} records, {n_runs} runs of N put in, written in {time.perf_counter() - t0:.1f} s", flush=True)

# stderr of the library (the debug lines) into a file
sys.stderr.flush()
saved = os.dup(2)
fd = os.open(log, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
os.dup2(fd, 2)
try:
    with MxEngine(k=32, w=1000) as eng:
        a = eng.add_fasta("t", 1.0, fa)
        reps = []
        for i in range(6):
            t = time.perf_counter()
            rep = eng.assembly_report(a)
            reps.append(time.perf_counter() - t)
            t = time.perf_counter()
            eng.write_fai(a, fa + ".fai")
            reps.append(time.perf_counter() - t)
        wall_rep, wall_fai = reps[2::2], reps[3::2]
        # scaffolds: 2 paths per record over most of the text
        L = int(lens[0])
        rows, first = [], [0]
        for r in range(N_REC):
            for p in range(2 if r != 8 else 0):
                base = p * (L // 2)
                rows.append((r, base + 1000, base + L // 4, 100, 0, 0, 0))
                rows.append((r, base + L // 4 + 500, base + L // 2 - 1000, 0, 0, 0, p))
                first.append(len(rows))
        names = [os.path.join(work, "m.assigned.fa"), os.path.join(work, "m.unassigned.fa"), os.path.join(work, "m.bed")]
        scaf = {False: [], True: []}
        for i in range(4):
            for flag in (False, True):
                t = time.perf_counter()
                eng.write_scaffolds(a, rows, first, assigned=names[0], unassigned=names[1], bed=names[2], report=flag)
                scaf[flag].append(time.perf_counter() - t)
        srep = eng.scaffold_report("all")
finally:
    sys.stderr.flush()
    os.dup2(saved, 2)
    os.close(fd)
text = open(log).read()
p1 = [tuple(float(x) for x in m) for m in re.findall(r"report items=\d+ pass1_ms=([\d.]+) scan_ms=([\d.]+) pass2_ms=([\d.]+)", text)]
items = re.findall(r"report items=(\d+)", text)
fai = [float(x) for x in re.findall(r"fai items=\d+ rows_ms=([\d.]+)", text)]
asm = p1[1:6]
med = lambda v: statistics.median(v)  # noqa: E731
print(f"assembly_report items={items[0]} device ms (median of 5 after a warm-up): pass1 {med([x[0] for x in asm]):.3f} scan {med([x[1] for x in asm]):.3f} "
      f"pass2 {med([x[2] for x in asm]):.3f} total {med([sum(x) for x in asm]):.3f}; all: {asm}")
print(f"write_fai text pass + scan device ms (median of 5 after a warm-up): {med(fai[1:6]):.3f}; all: {fai[:6]}")
print(f"wall: assembly_report {med(wall_rep) * 1e3:.2f} ms, write_fai {med(wall_fai) * 1e3:.2f} ms (with its file)")
print(f"text bytes {size}: pass 1 reads them once -> {size / med([x[0] for x in asm]) / 1e6:.1f} GB/s; fai {size / med(fai[1:6]) / 1e6:.1f} GB/s")
print(f"report: records {rep['n_records']} bases {rep['bases']} gaps {rep['n_gaps']} max_gap {rep['max_gap']} N {rep['n']} contigs {rep['contig']['n']} "
      f"N50 {rep['scaffold']['n50']} ctg_N50 {rep['contig']['n50']}")
print(f"write_scaffolds wall s: without {[round(x, 3) for x in scaf[False]]} with {[round(x, 3) for x in scaf[True]]}; medians of the last 3: "
      f"{med(scaf[False][1:]):.3f} / {med(scaf[True][1:]):.3f}; files {os.path.getsize(names[0])} + {os.path.getsize(names[1])} bytes")
win = p1[6:]
print(f"scaffold windows with the flag: {len(win)} passes; per call device ms pass1+scan+pass2 = {sum(sum(x) for x in win) / 4:.2f}")
print(f"scaffold report: records {srep['n_records']} bases {srep['bases']} gaps {srep['n_gaps']}")
for n in [fa, fa + ".fai", log] + names:
    os.remove(n)
os.rmdir(work)
