"""What a `bgzip`-compressed FASTA costs on the file route, against the plain file and against the host-zlib route of the commit
before: python tools/bgzf_rate.py [mbp] [threads] [runs] [out.txt].  Not a test.

One synthetic assembly of `mbp` Mbp (mxg_synth_write_fasta, default 1000) is written once and compressed once to BGZF (members of
65 280 bytes, zlib level 6 as bgzip's default, tests/_bgzf.py in a process pool of at most 16).  Timed is MxEngine.add_fasta, the call
that ends with the bases packed in HBM and the run table built, for
  (a) the plain file, this build            (a0) the plain file, the build in ab/base (the parent commit, as tools/ab.sh lays it out)
  (b) the BGZF file, this build: inflated on the device
  (c) the BGZF file, ab/base: inflated by zlib on one host thread.
Every measurement is a child process of its own (the library is chosen by MXG_LIB_DIR when it is loaded): it first loads a small plain
file, which pays the pinned pool, the first allocations and the code objects, then times the one call.  `runs` rounds (default 5), the four
variants interleaved in every round, both files in the page cache from their writing.  MXG_DEBUG_IO=1 in the children gives the parser's
own phase line ("packed at") and the kernel's line (bgzf_inflate ... ms=): the inflate kernel's share of (b)."""
import multiprocessing
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PAYLOAD = 65280


def _members(args):
    from tests import _bgzf
    path, lo, hi = args
    with open(path, "rb") as fh:
        fh.seek(lo)
        data = fh.read(hi - lo)
    return b"".join(_bgzf.member(data[p:p + PAYLOAD]) for p in range(0, len(data), PAYLOAD))


def compress(fa, gz, workers):
    from tests import _bgzf
    size, piece = os.path.getsize(fa), 256 * PAYLOAD
    jobs = [(fa, lo, min(size, lo + piece)) for lo in range(0, size, piece)]
    # (fresh interpreters, not forks: the parent has the GPU open and its workers must not inherit that)
    with ProcessPoolExecutor(max_workers=workers, mp_context=multiprocessing.get_context("spawn")) as pool, open(gz, "wb") as out:
        for blob in pool.map(_members, jobs):
            out.write(blob)
        out.write(_bgzf.EOF_MARKER)


def child(warm, fa, threads):
    from ntjoin_amd.engine import MxEngine
    with MxEngine(k=32, w=1000, device=0, threads=threads) as eng:
        eng.add_fasta("warm", 1.0, warm)
        sys.stderr.write("[rate] timed call\n")
        sys.stderr.flush()
        t0 = time.perf_counter()
        eng.add_fasta("x", 1.0, fa)
        dt = time.perf_counter() - t0
        st = eng.stats()
    print(f"RESULT {dt:.4f} {int(st['bases'])}", flush=True)


def measure(label, lib_dir, warm, fa, threads):
    env = dict(os.environ, MXG_DEBUG_IO="1")
    env.pop("MXG_LIB_DIR", None)
    env.pop("MXG_HOST_INGEST", None)
    if lib_dir:
        env["MXG_LIB_DIR"] = lib_dir
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", warm, fa, str(threads)], env=env, capture_output=True, text=True,
                       timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"{label}: child failed ({r.returncode})\n{r.stderr[-3000:]}")
    dt, bases = re.search(r"RESULT ([0-9.]+) (\d+)", r.stdout).groups()
    timed = r.stderr.split("[rate] timed call\n", 1)[1]
    packed = re.search(r"load_fasta_device .*? packed at ([0-9.]+)", timed)
    inflate = re.search(r"bgzf_inflate members=(\d+) bytes_in=(\d+) bytes_out=(\d+) ms=([0-9.]+)", timed)
    return {"s": float(dt), "bases": int(bases), "packed_s": float(packed.group(1)) if packed else None,
            "inflate_ms": float(inflate.group(4)) if inflate else None}


def spread(v):
    return f"median {statistics.median(v):.3f}  min {min(v):.3f}  max {max(v):.3f}  (" + " ".join(f"{x:.3f}" for x in v) + ")"


def main():
    mbp = float(sys.argv[1]) if len(sys.argv) > 1 else 1000.0
    threads = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    out_path = sys.argv[4] if len(sys.argv) > 4 else None
    base = os.path.join(REPO, "ab", "base")
    if not os.path.exists(os.path.join(base, "libntjoin_mx.so")):
        raise SystemExit("ab/base/libntjoin_mx.so (the parent commit's build) is missing")
    import numpy as np
    import bench
    from ntjoin_amd import capi, synth
    cfg, asms, _ = bench.workload_tables("configs2", mbp, 1000, seed=1)
    lib = capi.load()
    td = tempfile.mkdtemp(prefix="mxg_bgzf_")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    try:
        name, weight, segs, n_words, sub, sub_seed = asms[0]
        d = synth.fill_device(segs, n_words, cfg["seed"], sub_seed, sub)
        words = d.cpu().numpy().view(np.uint32)
        fa, gz, warm = os.path.join(td, "ref.fa"), os.path.join(td, "ref.fa.gz"), os.path.join(td, "warm.fa")
        st, ln = np.ascontiguousarray(segs[:, 0]), np.ascontiguousarray(segs[:, 2])
        assert lib.mxg_synth_write_fasta(fa.encode(), words.ctypes.data, st.ctypes.data, ln.ctypes.data, len(ln), b"s", 80, 8) == 0
        del d, words
        with open(warm, "w") as fh:
            fh.write(">w\n" + "ACGTTGCAAC" * 20000 + "\n")
        t0 = time.perf_counter()
        compress(fa, gz, min(15, os.cpu_count() or 1))
        say(f"bgzf_rate: {mbp:g} Mbp, {threads} host threads, {runs} interleaved rounds; plain {os.path.getsize(fa) / 1e9:.3f} GB, "
            f"BGZF {os.path.getsize(gz) / 1e9:.3f} GB ({os.path.getsize(fa) / os.path.getsize(gz):.2f}x, written in {time.perf_counter() - t0:.1f} s)")
        variants = [("a  plain, this build", None, fa), ("a0 plain, parent build", base, fa), ("b  BGZF, this build (device inflate)", None, gz),
                    ("c  BGZF, parent build (host zlib)", base, gz)]
        res = {v[0]: [] for v in variants}
        for _ in range(runs):
            for label, lib_dir, path in variants:
                res[label].append(measure(label, lib_dir, warm, path, threads))
        bases = {r["bases"] for v in res.values() for r in v}
        assert len(bases) == 1, bases   # (every route packed the same number of bases)
        say("add_fasta, seconds:")
        for label, _, _ in variants:
            say(f"  {label:40s} {spread([r['s'] for r in res[label]])}")
        a, a0, b, c = (res[v[0]] for v in variants)
        say("of which until the bases are packed (the parser's own clock), seconds:")
        for label in (variants[0][0], variants[2][0]):
            say(f"  {label:40s} {spread([r['packed_s'] for r in res[label]])}")
        ms = [r["inflate_ms"] for r in b]
        say(f"  inflate kernel (+ the header count beside it), ms: {spread(ms)}")
        say(f"  its share of (b): {100 * statistics.median(ms) / 1e3 / statistics.median([r['s'] for r in b]):.1f} %")
        say(f"(b) faster than (c) in every round: {all(x['s'] < y['s'] for x, y in zip(b, c))}")
        lo, hi = min(r["s"] for r in a0), max(r["s"] for r in a0)
        say(f"(a) median {statistics.median([r['s'] for r in a]):.3f} within the parent's (a0) own spread [{lo:.3f}, {hi:.3f}]: "
            f"{lo <= statistics.median([r['s'] for r in a]) <= hi}")
        say(f"(b) faster than (a) in every round: {all(x['s'] < y['s'] for x, y in zip(b, a))}; medians {statistics.median([r['s'] for r in b]):.3f} vs "
            f"{statistics.median([r['s'] for r in a]):.3f}")
        if any(r["inflate_ms"] is not None for r in a + a0 + c) or any(r["inflate_ms"] is None for r in b):
            say("UNEXPECTED: the bgzf_inflate line appeared where the device did not inflate, or is missing where it did")
    finally:
        shutil.rmtree(td, ignore_errors=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    else:
        main()
