"""What writing the scaffold FASTA as BGZF costs against the plain files, and whether the plain route moved:
python tools/bgzf_deflate_rate.py [mbp] [runs] [out.txt].  Not a test; the counterpart of tools/bgzf_rate.py.

One synthetic target of `mbp` Mbp (default 1000; tools/time_scaffolds.py's input: lines of 80, a few runs of N, paths of three nodes
over most of it, overlap stage on) is written once.  Timed is mxg_write_scaffolds to regular files in the system's temporary
directory, for
  (a)  plain, this build         (a0) plain, the parent commit's tree in ab/base (its ntjoin_amd package with its lib/ inside)
  (b)  MXG_SCAF_BGZF, this build: deflated on the device.
Every measurement is a child process of its own: it loads the target, makes one call of the measured kind that is not timed (the
pinned pool, the allocations, the code objects), then times one call.  `runs` rounds (default 5), the variants interleaved in every
round.  MXG_DEBUG_IO=1 in the children gives the kernel's own line (bgzf_deflate ... ms=): the deflate and pack kernels' share of
(b).  For scale: `gzip -6` (Python's zlib) on a 64 MB excerpt of the assigned file, ratio and seconds on one core."""
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(tree, fasta, td, bgzf):
    sys.path.insert(0, tree)
    import numpy as np
    from ntjoin_amd.engine import MxEngine
    nodes, first = np.load(os.path.join(td, "nodes.npy")), np.load(os.path.join(td, "first.npy"))
    names = [os.path.join(td, f) for f in ("a.fa", "u.fa", "u.bed")]
    kw = {"bgzf": True} if bgzf else {}
    with MxEngine(k=32, w=1000) as eng:
        a = eng.add_fasta("t", 1.0, fasta)
        call = lambda: eng.write_scaffolds(a, nodes, first, overlap_gap=20, assigned=names[0], unassigned=names[1], bed=names[2], **kw)  # noqa: E731
        call()
        sys.stderr.write("[rate] timed call\n")
        sys.stderr.flush()
        t0 = time.perf_counter()
        call()
        dt = time.perf_counter() - t0
    print(f"RESULT {dt:.4f} {os.path.getsize(names[0])} {os.path.getsize(names[1])}", flush=True)


def measure(label, tree, fasta, td, bgzf):
    env = dict(os.environ, MXG_DEBUG_IO="1")
    for k in ("MXG_LIB_DIR", "MXG_SCAF_WIN", "MXG_BGZF_PAYLOAD"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, fasta, td, "1" if bgzf else "0"], env=env,
                       capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"{label}: child failed ({r.returncode})\n{r.stderr[-3000:]}")
    dt, n_a, n_u = re.search(r"RESULT ([0-9.]+) (\d+) (\d+)", r.stdout).groups()
    timed = r.stderr.split("[rate] timed call\n", 1)[1]
    lines = re.findall(r"bgzf_deflate members=(\d+) bytes_in=(\d+) bytes_out=(\d+) stored=(\d+) ms=([0-9.]+)", timed)
    return {"s": float(dt), "bytes": int(n_a) + int(n_u), "kernel_ms": sum(float(x[4]) for x in lines) if lines else None,
            "text": sum(int(x[1]) for x in lines) if lines else None, "members": sum(int(x[0]) for x in lines) if lines else None}


def spread(v):
    return f"median {statistics.median(v):.3f}  min {min(v):.3f}  max {max(v):.3f}  (" + " ".join(f"{x:.3f}" for x in v) + ")"


def main():
    mbp = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out_path = sys.argv[3] if len(sys.argv) > 3 else None
    base = os.path.join(REPO, "ab", "base")
    if not os.path.exists(os.path.join(base, "ntjoin_amd", "lib", "libntjoin_mx.so")):
        raise SystemExit("ab/base/ntjoin_amd (the parent commit's package with its built lib/) is missing")
    sys.path.insert(0, REPO)
    sys.path.insert(1, os.path.join(REPO, "tools"))
    import time_scaffolds
    td = tempfile.mkdtemp(prefix="mxg_deflate_")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    try:
        fasta = os.path.join(td, "t.fa")
        import numpy as np
        _, nodes, first = time_scaffolds.make_input(mbp, fasta)
        np.save(os.path.join(td, "nodes.npy"), nodes)
        np.save(os.path.join(td, "first.npy"), first)
        variants = [("a  plain, this build", REPO, False), ("a0 plain, parent build", base, False), ("b  BGZF, this build (device deflate)", REPO, True)]
        res = {v[0]: [] for v in variants}
        for _ in range(runs):
            for label, tree, bgzf in variants:
                res[label].append(measure(label, tree, fasta, td, bgzf))
                if not bgzf and tree == REPO:   # the plain assigned file of this round: an excerpt for gzip's ratio
                    with open(os.path.join(td, "a.fa"), "rb") as fh:
                        excerpt = fh.read(64 << 20)
        a, a0, b = (res[v[0]] for v in variants)
        text = a[0]["bytes"]
        say(f"bgzf_deflate_rate: target of {mbp} Mbp, {runs} interleaved rounds, regular files in {tempfile.gettempdir()}; scaffold text "
            f"{text / 1e9:.3f} GB (assigned + unassigned)")
        say("mxg_write_scaffolds, seconds:")
        for label, _, _ in variants:
            say(f"  {label:40s} {spread([r['s'] for r in res[label]])}")
        say("bytes written (the two FASTA files):")
        for label, _, _ in variants:
            say(f"  {label:40s} {res[label][0]['bytes']}")
        assert b[0]["text"] == text and a0[0]["bytes"] == text, (b[0]["text"], a0[0]["bytes"], text)
        ms = [r["kernel_ms"] for r in b]
        say(f"  deflate + scan + pack kernels of (b), ms: {spread(ms)}  ({b[0]['members']} members)")
        say(f"  their share of (b): {100 * statistics.median(ms) / 1e3 / statistics.median([r['s'] for r in b]):.1f} %")
        t0 = time.perf_counter()
        z = len(zlib.compress(excerpt, 6))
        dt = time.perf_counter() - t0
        say(f"compressed size / text size: BGZF from the device {b[0]['bytes'] / text:.4f}; gzip -6 (zlib, one core) on a {len(excerpt) / 1e6:.0f} MB excerpt "
            f"{z / len(excerpt):.4f} in {dt:.2f} s = {len(excerpt) / dt / 1e6:.0f} MB/s")
        ma, mb = statistics.median([r["s"] for r in a]), statistics.median([r["s"] for r in b])
        say(f"(b) against (a): medians {mb:.3f} vs {ma:.3f} s ({ma / mb:.2f}x); (b) faster in every round: {all(x['s'] < y['s'] for x, y in zip(b, a))}; "
            f"(a) faster in every round: {all(y['s'] < x['s'] for x, y in zip(b, a))}")
        lo, hi = min(r["s"] for r in a0), max(r["s"] for r in a0)
        say(f"(a) median {ma:.3f} within the parent's (a0) own spread [{lo:.3f}, {hi:.3f}]: {lo <= ma <= hi}")
        if any(r["kernel_ms"] is not None for r in a + a0) or any(r["kernel_ms"] is None for r in b):
            say("UNEXPECTED: the bgzf_deflate line appeared where the device did not deflate, or is missing where it did")
    finally:
        shutil.rmtree(td, ignore_errors=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5] == "1")
    else:
        main()
