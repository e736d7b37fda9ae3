"""time the identity of the synteny blocks (mxg_synteny_identity):
    MXG_DEBUG_IO=1 python tools/time_identity.py [--mbp 3000] [--dir DIR]
    MXG_DEBUG_IO=1 MXG_IDY_ORDER=0 python tools/time_identity.py        (the lanes' segments in list order, without the sort by length)
On the configs[2]-shaped pair of bench.py (3 Gbp reference of 24 records + derived target, k=32, w=1000), written out as FASTA of 80
columns so that the handle holds its text: three blocks calls and three identity calls of the target on the reference, then the same
through the piece table of scaffolds kept on the device (pairs of neighbouring contigs, the second reversed, 100 N between them).
The library prints the device time of every call (HIP events) on stderr; the wall time of every call and the shares of segments and of
bases under every skip rule are printed here.  The first call of each pays its allocations.  About 2 x mbp MB of scratch files."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from ntjoin_amd import capi, synth  # noqa: E402
from ntjoin_amd.engine import MxEngine  # noqa: E402


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    return (time.perf_counter() - t0) * 1e3, res


def shares(res):
    n, q = max(res["n_segments"], 1), max(res["block_q"], 1)
    return (f"{res['n_blocks']} blocks, {res['n_segments']} segments: aligned {100 * res['n_aligned'] / n:.3f} % (saturated "
            f"{100 * res['n_saturated'] / n:.4f} %), skipped by length {100 * res['n_skip_len'] / n:.4f} %, by shift {100 * res['n_skip_shift'] / n:.4f} %, "
            f"by class 4 {100 * res['n_skip_n'] / n:.4f} %; aligned query bases {100 * res['aligned_q'] / q:.3f} % of {res['block_q']}; "
            f"edits {res['edits']} = {1e5 * res['edits'] / max(res['aligned_q'], res['aligned_s'], 1):.2f} per 100 kbp")


ap = argparse.ArgumentParser()
ap.add_argument("--mbp", type=int, default=3000)
ap.add_argument("--dir", default=None, help="where the two FASTA files go (default: the system's temporary directory)")
args = ap.parse_args()
lib = capi.load()
with tempfile.TemporaryDirectory(dir=args.dir) as td, MxEngine(k=32, w=1000) as eng:
    cfg = synth.genome_config(args.mbp * 1_000_000, 24, seed=1, min_len=3000, max_len=600_000)
    for which, name, weight in (("ref", "ref", 2.0), ("tgt", "tgt", 1.0)):
        segs, n_words = cfg[which + "_segs"], cfg[which + "_words"]
        d = synth.fill_device(segs, n_words, cfg["seed"], cfg["sub_seed"], synth.SUB_PER_65536 if which == "tgt" else 0)
        words = d.cpu().numpy().view(np.uint32)
        fa = os.path.join(td, name + ".fa")
        st, ln = np.ascontiguousarray(segs[:, 0]), np.ascontiguousarray(segs[:, 2])
        assert lib.mxg_synth_write_fasta(fa.encode(), words.ctypes.data, st.ctypes.data, ln.ctypes.data, len(ln), b"s", 80, 16) == 0
        del d, words
        torch.cuda.empty_cache()
        t0 = time.perf_counter()
        eng.add_fasta(name, weight, fa)
        print(f"{name}: {os.path.getsize(fa) / 1e9:.2f} GB of FASTA loaded in {time.perf_counter() - t0:.1f} s", flush=True)
        os.remove(fa)
    eng.sketch()
    eng.build_graph()
    lengths = eng.record_lengths(1)
    n = len(lengths) // 2 * 2
    rows = [(c, 0, int(lengths[c]), 100 if c % 2 == 0 else 0, 0, 0, c % 2) for c in range(n)]
    eng.write_scaffolds(1, rows, list(range(0, n + 1, 2)), keep=True)
    pieces, first, _ids = eng.scaffold_pieces()
    for what, kw in (("target on reference", {}), ("scaffolds on reference, through the kept text's table", dict(pieces=pieces, first=first))):
        for rep in range(3):
            ms_b, blocks = wall_ms(lambda: eng.synteny_blocks(1, 0, **kw))
            ms_i, res = wall_ms(eng.synteny_identity)
            print(f"{what}, call {rep + 1}: blocks {ms_b:.2f} ms wall ({blocks['n_blocks']} kept of {blocks['n_anchors_total']} anchors), "
                  f"identity {ms_i:.2f} ms wall", flush=True)
        print(f"{what}: {shares(res)}", flush=True)
    print("knobs:", eng.knobs(), flush=True)
