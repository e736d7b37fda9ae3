"""time the path adjustment stage in one call (mxg_adjust_paths): python tools/time_adjust_paths.py [--no-pair]
Median of 5 calls after one warm-up of MxEngine.adjust_paths (arrays in, arrays back) beside one run of the Python restatement
(tests/_adjust_restatement.py, the checker) on the same rows, which are compared:
  (1) the 10^5-node case of the tests (tests/_adjust_cases.large_case), with and without no_cut
  (2) the nodes of a configs[2]-shaped pair (3 Gbp reference of 24 records + derived target, w=1000) after find_paths(2) and
      MxEngine.format_paths; how many nodes the call merged or dropped there is printed too.  --no-pair leaves (2) out."""
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from ntjoin_amd.engine import MxEngine  # noqa: E402
from tests import _adjust_cases as cases, _adjust_restatement as rs  # noqa: E402


def median_ms(fn, reps=5):
    fn()
    out, res = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), res


def report(eng, label, paths, no_cut, G):
    nodes, first, names = cases.to_arrays(paths, MxEngine.ADJUST_NODE)
    try:
        rs.adjust(paths, no_cut, G)
    except KeyError as key:  # (the reference raises there, the library refuses: nothing to time)
        print(f"{label}, no_cut={no_cut}: KeyError at (path, node) {key.args[0]}")
        return
    ms, res = median_ms(lambda: eng.adjust_paths(nodes, first, no_cut=no_cut, G=G))
    res["in_first"] = first
    t0 = time.perf_counter()
    want = rs.adjust(paths, no_cut, G)
    ms_py = (time.perf_counter() - t0) * 1e3
    got = cases.from_arrays(res, names)
    assert (got[0], got[1]) == want, "the library's rows differ from the restatement's"
    changed = sum(1 for path_in, path_out in zip(paths, want[0]) for row in path_out if row not in path_in)
    print(f"{label}, no_cut={no_cut}: {len(nodes)} nodes in {len(paths)} paths over {len(names)} contigs -> {len(res['nodes'])} nodes "
          f"({changed} changed): mxg_adjust_paths {ms:.2f} ms, restatement {ms_py:.0f} ms")


with MxEngine(k=32, w=1000) as eng:
    large = cases.large_case()
    for no_cut in (False, True):
        report(eng, "10^5-node case", large["paths"], no_cut, 0)
    if "--no-pair" not in sys.argv:
        import torch  # noqa: F401  (the synthetic genomes are filled into torch tensors)
        from ntjoin_amd import synth
        cfg = synth.genome_config(3_000_000_000, 24, seed=1, min_len=3000, max_len=600_000)
        for which, name, weight in (("ref", "ref", 2.0), ("tgt", "tgt", 1.0)):
            segs, n_words = cfg[which + "_segs"], cfg[which + "_words"]
            d = synth.fill_device(segs, n_words, cfg["seed"], cfg["sub_seed"], synth.SUB_PER_65536 if which == "tgt" else 0)
            eng.add_packed_device(name, weight, d.data_ptr(), segs[:, 0], segs[:, 2], keepalive=d)
        eng.sketch(-2)
        eng.build_graph()
        found = eng.find_paths(2)
        ids = eng.record_ids(1, eng.n_records(1))
        nd = eng.format_paths(1, g=20, G=0, m=90, mkt=False)
        # rows as Ntjoin.format_paths makes them, the vertex indices standing in for the minimizer hashes (opaque tags to this stage)
        rows = [list(r) for r in zip(
            [ids[r] for r in nd["record"].tolist()], ["-" if r else "+" for r in nd["reverse"].tolist()], nd["start"].tolist(),
            nd["end"].tolist(), nd["contig_size"].tolist(), map(str, nd["first_vertex"].tolist()), map(str, nd["terminal_vertex"].tolist()),
            nd["gap_size"].tolist(), nd["raw_gap_size"].tolist())]
        at = nd["node_first"].tolist()
        paths = [rows[lo:hi] for lo, hi in zip(at, at[1:])]
        per_contig = np.unique([row[0] for path in paths for row in path], return_counts=True)[1]
        print(f"configs[2] pair, -n 2: {len(found)} paths, {int((per_contig > 1).sum())} contigs in more than one node")
        for no_cut in (False, True):
            report(eng, "configs[2] pair", paths, no_cut, 0)
