"""time the assessment beside the blocks call (mxg_synteny_blocks, mxg_synteny_assess):
    MXG_DEBUG_IO=1 python tools/time_assess.py
On the configs[2]-shaped pair of bench.py (3 Gbp reference of 24 records + derived target, k=32, w=1000) on one handle: three blocks
calls and three assess calls of the target on the reference, then the same through a table of one piece per contig, every other one
REV.  The library prints the device time of every call (HIP events) on stderr; the wall time of every call is printed here.  The
first call of each pays its allocations."""
import sys
import time

import torch

sys.path.insert(0, ".")
from ntjoin_amd import synth  # noqa: E402
from ntjoin_amd.engine import MxEngine  # noqa: E402


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    return (time.perf_counter() - t0) * 1e3, res


with MxEngine(k=32, w=1000) as eng:
    cfg = synth.genome_config(3_000_000_000, 24, seed=1, min_len=3000, max_len=600_000)
    for which, name, weight in (("ref", "ref", 2.0), ("tgt", "tgt", 1.0)):
        segs, n_words = cfg[which + "_segs"], cfg[which + "_words"]
        d = synth.fill_device(segs, n_words, cfg["seed"], cfg["sub_seed"], synth.SUB_PER_65536 if which == "tgt" else 0)
        eng.add_packed_device(name, weight, d.data_ptr(), segs[:, 0], segs[:, 2], keepalive=d)
    eng.sketch(-2)
    eng.build_graph()
    lengths = eng.record_lengths(1)
    table = dict(pieces=[(r, 0, ln, r % 2) for r, ln in enumerate(lengths)], first=list(range(len(lengths) + 1)))
    for what, kw in (("target on reference", {}), ("through a table of one piece per contig", table)):
        for rep in range(3):
            ms_b, blocks = wall_ms(lambda: eng.synteny_blocks(1, 0, **kw))
            ms_a, res = wall_ms(eng.synteny_assess)
            print(f"{what}, call {rep + 1}: blocks {ms_b:.2f} ms wall ({blocks['n_blocks']} kept of {blocks['n_anchors_total']} anchors), "
                  f"assess {ms_a:.2f} ms wall ({res['n_chains']} chains, {res['n_breakpoints']} breakpoints, NGA50 {res['nga']['n50']}, "
                  f"covered {res['covered_subject']} of {res['subject_bases']})", flush=True)
