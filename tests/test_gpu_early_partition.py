"""GPU test of the fused call's early partitioning: mxg_sketch_graph lays the two-level join out before the first filter is
launched and partitions every assembly behind its own k_emit, into its own sub-range of every coarse partition (graph_join
| 0x400).  Whatever the inputs, the call must hand back what mxg_sketch + mxg_build_graph do, what it does with
MXG_PJ_EARLY=0 (today's order: partitioned behind the last sketch), and what the global-table join does; on the way out
of the common case (a forced join failure, a sub-range that overflows, a batch that does not end well, several batches)
nothing of the early kernels may be left in the result."""
import os
import tempfile

import numpy as np
import pytest

from ntjoin_amd import synth

pytestmark = pytest.mark.gpu

K, W = 32, 200
EARLY = 0x400
KNOBS = ("MXG_PJ_TWO_LEVEL", "MXG_PJ_EARLY", "MXG_PJ_FORCE_FAIL", "MXG_GRAPH_JOIN", "MXG_SEL_BATCH_KMERS")


def _state(eng, n_asm):
    out = {}
    for a in range(n_asm):
        sk = eng.get_sketch(a)
        for key in ("out_hash", "pos", "record", "forward", "record_first"):
            out[f"{key}{a}"] = np.array(sk[key], copy=True)
        out[f"flags{a}"] = np.array(eng.get_mx_flags(a), copy=True)
    for key, val in eng.get_graph().items():
        out[key] = np.array(val, copy=True)
    st = eng.stats()
    for key in ("minimizers", "unique", "vertices", "edges"):
        out[key] = np.array([st[key]])
    return out


def _same(x, y, what):
    assert x.keys() == y.keys(), what
    for key in x:
        assert np.array_equal(x[key], y[key]), (what, key)


class _Env:
    """the knobs of one engine: a handle reads each at its first use, so they stay set while the engine works"""

    def __init__(self, **env):
        self.env = env

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in KNOBS}
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _add(eng, asms):
    for name, weight, recs in asms:
        eng.add_records(name, weight, [(f"r{i}", synth.to_ascii(c)) for i, c in enumerate(recs)])


def _run(asms, fused, steps=1, w=W, **env):
    """-> (state, graph_join of every step)"""
    from ntjoin_amd.engine import MxEngine
    joins = []
    with _Env(**env), MxEngine(k=K, w=w) as eng:
        _add(eng, asms)
        for _ in range(steps):
            if fused:
                eng.sketch_graph()
            else:
                eng.sketch(-2)
                eng.build_graph()
            joins.append(int(eng.stats()["graph_join"]))
        return _state(eng, len(asms)), joins


def _four_ways(asms, w=W, **env):
    """the early path against the two calls, MXG_PJ_EARLY=0 and the global table; -> (state, graph_join) of the early path"""
    early, joins = _run(asms, True, w=w, MXG_PJ_TWO_LEVEL="1", **env)
    _same(early, _run(asms, False, w=w, MXG_PJ_TWO_LEVEL="1", **env)[0], "two calls")
    late, jl = _run(asms, True, w=w, MXG_PJ_TWO_LEVEL="1", MXG_PJ_EARLY="0", **env)
    assert not (jl[0] & EARLY), hex(jl[0])
    _same(early, late, "MXG_PJ_EARLY=0")
    _same(early, _run(asms, False, w=w, MXG_GRAPH_JOIN="global")[0], "global table")
    return early, joins[0]


def _pieces(ref, seed, lo, hi, **kw):
    """a target derived from bases [lo, hi) of the reference's first record"""
    return synth.derive_target([ref[0][lo:hi]], seed, min_len=5_000, max_len=200_000, **kw)


def _family(n_asm, with_empty):
    ref = synth.make_reference(31, 6_000_000, 2)
    sizes = [(0, 3_000_000), (900_000, 1_300_000), (1_000_000, 1_100_000), (500_000, 2_000_000)]
    asms = [("ref", 2.0, ref)]
    for i in range(n_asm - 1):
        lo, hi = sizes[i % len(sizes)]
        asms.append((f"t{i}", 1.0 + i / 4, _pieces(ref, 40 + i, lo, hi)))
    if with_empty:
        asms[1] = ("empty", 1.0, [np.zeros(20, dtype=np.uint8)])  # shorter than a window: no minimizer
    return asms


def _check_against_oracle(asms):
    """the early path's .mx.dot against oracle/graph_oracle.py, as smoke() does it"""
    from ntjoin_amd.engine import MxEngine
    from oracle import graph_oracle
    with _Env(MXG_PJ_TWO_LEVEL="1"), tempfile.TemporaryDirectory() as td, MxEngine(k=K, w=W) as eng:
        names = [os.path.join(td, f"{name}.fa.k{K}.w{W}.tsv") for name, _, _ in asms]
        _add(eng, [(path, wt, recs) for path, (_, wt, recs) in zip(names, asms)])  # (the assemblies go by their files' names, as in ntJoin)
        eng.sketch_graph()
        assert eng.stats()["graph_join"] & EARLY
        for a, path in enumerate(names):
            eng.write_tsv(a, path)
        eng.write_dot(os.path.join(td, "out.mx.dot"))
        state = graph_oracle.load_and_build(names[:-1], [wt for _, wt, _ in asms[:-1]], names[-1], asms[-1][1])
        with open(os.path.join(td, "out.mx.dot"), encoding="utf-8") as fh:
            got = graph_oracle.canonical_dot_from_text(fh.read())
        assert got == graph_oracle.canonical_dot_from_state(state)


@pytest.mark.parametrize("n_asm,with_empty", [(2, False), (3, False), (5, False), (3, True)])
def test_unequal_assemblies(n_asm, with_empty):
    """with_empty: an assembly without a minimizer never reaches the streams, so the join is NOT planned early and the graph has no
    vertex -- the case pins that the call still answers like the others, it is no coverage of an empty sub-range (those are
    written by k_pj2_bucket for every small assembly of the other cases)"""
    asms = _family(n_asm, with_empty)
    state, join = _four_ways(asms)
    if with_empty:
        assert state["vertices"][0] == 0      # (an empty assembly never reaches the streams: the stage runs on its own)
        assert not (join & EARLY), hex(join)
    else:
        assert state["vertices"][0] > 100
        assert join == 2 | EARLY, hex(join)
    if n_asm == 2:
        _check_against_oracle(asms)


def test_forced_join_failure_drops_the_early_partitions():
    asms = _family(3, False)
    state, join = _four_ways(asms, MXG_PJ_FORCE_FAIL="1")
    assert join == 3 | 0x200, hex(join)       # the global table ran, and its result is the one that stays
    assert state["vertices"][0] > 100


def _periodic_unit(orc, period, want, split=None):
    """a random unit whose tandem array has exactly `want` minimizers per copy, dealt as `split` (default: all in one) over the
    two coarse partitions that MXG_PJ_TWO_LEVEL=1 makes of a small input (bit 52 of hash x 0x9E3779B97F4A7C15: pj1_part)"""
    split = split or (0, want)
    for seed in range(1000, 4000):
        unit = np.random.default_rng(seed).integers(0, 4, size=period, dtype=np.uint8)
        sk = orc.sketch(synth.to_ascii(np.tile(unit, 8)), K, W)
        hs = [h for h, p, _, _ in sk if 3 * period <= p < 4 * period]
        bits = [(((h * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF) >> 52) & 1 for h in set(hs)]
        if len(hs) == want and len(bits) == want and tuple(sorted((bits.count(0), bits.count(1)))) == tuple(split):
            return unit
    raise AssertionError("no unit found")


def test_sub_range_overflow_is_learnt():
    """95 % of one assembly is a tandem array of a 300-base unit with three minimizers per copy, all three in one coarse
    partition: ~190 000 of the assembly's ~200 000 records want a sub-range sized for 5/8 of its bound (230 000 / 2 x 1.25).
    The stage notices (| 0x100), sizes the sub-range by what the cursors counted, and the next call goes through early."""
    from ntjoin_amd.engine import MxEngine
    from tests import _oracle
    unit = _periodic_unit(_oracle.load(), 300, 3)
    plain = synth.make_reference(77, 1_000_000, 1)
    heavy = [plain[0], np.tile(unit, 19_000_000 // 300)]
    other = _pieces(plain, 78, 0, 1_000_000) + [np.tile(unit, 3)]
    asms = [("heavy", 2.0, heavy), ("other", 1.0, other)]
    want = _run(asms, False, MXG_GRAPH_JOIN="global")[0]
    assert want["vertices"][0] > 100
    with _Env(MXG_PJ_TWO_LEVEL="1"), MxEngine(k=K, w=W) as eng:
        _add(eng, asms)
        eng.sketch_graph()
        assert eng.stats()["graph_join"] == 2 | 0x100, hex(eng.stats()["graph_join"])
        _same(_state(eng, 2), want, "first call")
        eng.sketch_graph()
        assert eng.stats()["graph_join"] == 2 | EARLY, hex(eng.stats()["graph_join"])
        _same(_state(eng, 2), want, "second call")
    _same(_run(asms, True, MXG_PJ_TWO_LEVEL="1", MXG_PJ_EARLY="0")[0], want, "MXG_PJ_EARLY=0")


def test_batch_that_does_not_end_well():
    """two candidates per window leave candidate-free stretches all over both assemblies; the one-call mode cannot keep such a
    batch (its counts are already in use on the device), so after the early kernels have run behind both k_emit the sketches
    are redone and the graph stage partitions again from scratch: batches redone, no 0x400, and the result of the two calls"""
    from ntjoin_amd.engine import MxEngine
    ref, tgt = synth.config2(seed=4, n_bases=3_000_000)
    asms = [("ref", 2.0, ref), ("tgt", 1.0, tgt)]
    with _Env(MXG_PJ_TWO_LEVEL="1"), MxEngine(k=K, w=W, cand_per_window=2) as eng:
        _add(eng, asms)
        for step in range(2):  # (the second step starts from what the first one's early kernels left behind)
            before = eng.stats()
            eng.sketch_graph()
            st = eng.stats()
            assert st["batches_redone"] - before["batches_redone"] == 2 and st["sync_assemblies"] - before["sync_assemblies"] == 2, (step, st)
            assert st["graph_join"] == 2, (step, hex(st["graph_join"]))
            got = _state(eng, 2)
            if step == 0:
                first = got
        _same(got, first, "second step")
    _same(got, _run(asms, False, MXG_PJ_TWO_LEVEL="1")[0], "two calls")
    _same(got, _run(asms, False, MXG_GRAPH_JOIN="global")[0], "global table")
    assert got["vertices"][0] > 100


def test_sketch_that_outgrows_its_bound():
    """90 % of one assembly is a tandem array with four minimizers per 300 bases, two in either coarse partition: 260 000
    minimizers where the graph stage was laid out for 2.3 per window (231 000).  Every batch ends well and the early kernels run,
    but the stage behind them saw a cut-off sketch: the call drops it and builds the graph again on its own (no 0x400, nothing
    redone in the sketches).  The next call knows the size and goes through early."""
    from ntjoin_amd.engine import MxEngine
    from tests import _oracle
    unit = _periodic_unit(_oracle.load(), 300, 4, (2, 2))
    plain = synth.make_reference(91, 2_000_000, 1)
    dense = [plain[0], np.tile(unit, 18_000_000 // 300)]
    other = _pieces(plain, 92, 0, 2_000_000) + [np.tile(unit, 3)]
    asms = [("dense", 2.0, dense), ("other", 1.0, other)]
    want = _run(asms, False, MXG_GRAPH_JOIN="global")[0]
    assert want["vertices"][0] > 100 and want["out_hash0"].size > 2.3 * 20_000_000 / (W + 1) + 2048
    with _Env(MXG_PJ_TWO_LEVEL="1"), MxEngine(k=K, w=W) as eng:
        _add(eng, asms)
        eng.sketch_graph()
        st = eng.stats()
        assert st["graph_join"] & ~0x100 == 2, hex(st["graph_join"])
        assert st["batches_redone"] == 0 and st["sync_assemblies"] == 0 and st["retried_assemblies"] == 0, st
        _same(_state(eng, 2), want, "first call")
        eng.sketch_graph()
        assert eng.stats()["graph_join"] == 2 | EARLY, hex(eng.stats()["graph_join"])
        _same(_state(eng, 2), want, "second call")


def test_steps_back_to_back_then_one_more_assembly():
    from ntjoin_amd.engine import MxEngine
    ref = synth.make_reference(51, 4_000_000, 1)
    asms = [("ref", 2.0, ref), ("t0", 1.0, _pieces(ref, 52, 0, 2_500_000)), ("t1", 1.5, _pieces(ref, 53, 1_000_000, 4_000_000))]
    with _Env(MXG_PJ_TWO_LEVEL="1"), MxEngine(k=K, w=W) as eng:
        _add(eng, asms[:2])
        for step in range(2):
            eng.sketch_graph()
            assert eng.stats()["graph_join"] == 2 | EARLY, (step, hex(eng.stats()["graph_join"]))
        two = _state(eng, 2)
        _add(eng, asms[2:])
        eng.sketch_graph()
        assert eng.stats()["graph_join"] == 2 | EARLY, hex(eng.stats()["graph_join"])
        three = _state(eng, 3)
    _same(two, _run(asms[:2], False, MXG_PJ_TWO_LEVEL="1")[0], "two assemblies")
    _same(two, _run(asms[:2], False, MXG_GRAPH_JOIN="global")[0], "two assemblies, global table")
    _same(three, _run(asms, False, MXG_PJ_TWO_LEVEL="1")[0], "three assemblies")
    _same(three, _run(asms, True, MXG_PJ_TWO_LEVEL="1", MXG_PJ_EARLY="0")[0], "three assemblies, MXG_PJ_EARLY=0")
    assert three["vertices"][0] > 100


def test_assembly_of_several_batches():
    ref, tgt = synth.config2(seed=5, n_bases=12_000_000)
    asms = [("ref", 2.0, ref), ("tgt", 1.0, tgt)]
    state, join = _four_ways(asms, w=1000, MXG_SEL_BATCH_KMERS="3000000")
    assert not (join & EARLY), hex(join)
    assert state["vertices"][0] > 100
