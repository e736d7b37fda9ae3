"""time the path stage in one call (mxg_format_paths): python tools/time_format_paths.py
On a configs[2]-shaped pair (3 Gbp reference of 24 records + derived target, w=1000), after find_paths(2) on one handle, best of 5:
  (1) Ntjoin._format_paths_host   the host loop the call replaces (graph to the host, one dict entry per edge, a name per vertex)
  (2) MxEngine.format_paths       the library call, arrays back
  (3) Ntjoin.format_paths         the library call and the rows made from its arrays
once with mkt=False and once with mkt=True; the rows of (1) and (3) are compared.  (2) and (3) are timed first, before anything asks
for the graph's host mirror, which (1) needs and a run through the library never makes; its cost is printed beside the times.
--lib-only: (2) and (3) alone (for a kernel trace)."""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from ntjoin_amd import synth  # noqa: E402
from ntjoin_amd.engine import MxEngine  # noqa: E402
from ntjoin_amd.ntjoin import Ntjoin  # noqa: E402


def best_ms(fn, reps=5):
    out, res = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return min(out), res


with MxEngine(k=32, w=1000) as eng:
    cfg = synth.genome_config(3_000_000_000, 24, seed=1, min_len=3000, max_len=600_000)
    for which, name, weight in (("ref", "ref", 2.0), ("tgt", "tgt", 1.0)):
        segs, n_words = cfg[which + "_segs"], cfg[which + "_words"]
        d = synth.fill_device(segs, n_words, cfg["seed"], cfg["sub_seed"], synth.SUB_PER_65536 if which == "tgt" else 0)
        eng.add_packed_device(name, weight, d.data_ptr(), segs[:, 0], segs[:, 2], keepalive=d)
    eng.sketch(-2)
    eng.build_graph()
    found = eng.find_paths(2)
    ids = eng.record_ids(1, eng.n_records(1))
    lengths = dict(zip(ids, eng.record_lengths(1)))
    nj = Ntjoin.__new__(Ntjoin)
    nj.args = type("Args", (), {"k": 32})()
    nj._engine, nj._order, nj._found, nj._graph, nj._graph_pending = eng, ["ref", "tgt"], found, None, True
    lens = [lengths[c] for c in ids]
    lib = {}
    for mkt in (False, True):  # the library routes first: the graph has no host mirror yet, as in a run that never asks for one
        ms_lib, nodes = best_ms(lambda: eng.format_paths(1, g=20, G=0, m=90, mkt=mkt, lengths=lens))
        ms_rows, got = best_ms(lambda: nj.format_paths(lengths, 20, 0, 90, mkt))
        lib[mkt] = (ms_lib, ms_rows, nodes, got)
    if "--lib-only" in sys.argv:
        print({m: v[:2] for m, v in lib.items()})
        sys.exit(0)
    t0 = time.perf_counter()
    g = eng.get_graph()
    ms_mirror = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    _ = nj.graph.names[0]
    print(f"configs[2] pair, -n 2: {len(g['vertex_hash'])} vertices, {len(g['edge_u'])} edges, {len(found)} paths; once per handle, outside "
          f"the times below and needed by the host route only: graph to the host {ms_mirror:.0f} ms, array-backed graph object "
          f"{(time.perf_counter() - t0) * 1e3:.0f} ms")
    for mkt in (False, True):
        ms_lib, ms_rows, nodes, got = lib[mkt]
        ms_host, want = best_ms(lambda: nj._format_paths_host(lengths, 20, 0, 90, mkt))
        assert got == want, "the library's rows differ from the host route's"
        seg = eng.path_segments(1)
        sg, nf = nodes["segment"].astype(np.int64), nodes["node_first"].astype(np.int64)
        last = np.zeros(len(sg), dtype=bool)
        last[nf[1:][nf[1:] > nf[:-1]] - 1] = True
        j = np.flatnonzero(~last)
        first, n = seg["first"].astype(np.int64), seg["n"].astype(np.int64)
        stretch = first[sg[j + 1]] - (first[sg[j]] + n[sg[j]] - 1) if len(j) else np.zeros(0, dtype=np.int64)
        print(f"mkt={mkt}: {len(n)} runs, {len(sg)} nodes, {len(j)} junctions (longest stretch {int(stretch.max()) if len(j) else 0} edges, "
              f"{int((stretch > 1).sum())} longer than one): _format_paths_host {ms_host:.1f} ms, MxEngine.format_paths {ms_lib:.2f} ms, "
              f"Ntjoin.format_paths {ms_rows:.2f} ms")
