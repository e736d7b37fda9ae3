"""GPU test of the rank route of the graph stage's edge passes (k_edge_flags_rank, k_edges_rank in csrc/graph.hip; the predicate:
csrc/graph_rank.h): behind an LDS join the whole stage builds no adjacency table, k_vertices_pj stores the place of every vertex
in every assembly's filtered order and the edge passes decide "v is next to u in assembly b" from two places and two records.
MXG_GRAPH_RANK=0 restores k_adjacency and the table's passes.

Every case goes through add_minimizers + build_graph (small lists: the LDS join is taken) and is built twice, MXG_GRAPH_RANK at 1
and at 0.  Both builds must give the same vertex and edge arrays, those must be the C oracle's graph (tests/_oracle.py), and the
MXG_DEBUG_JOIN line must name the route that ran.  The shapes are the smallest at which the route can go wrong: the hand cases of
tests/test_graph_rank_cpu.py, vertex counts around a 256-block and a thread block of four at every width, a vertex count below
the rows' stride, every mask form (up to 4, up to 8, beyond 8 assemblies), a fuzz of kept, reversed and shuffled records, and the
fused call, where the counts are still on the device."""
import re

import numpy as np
import pytest

from tests import _oracle
from tests.test_graph_rank_cpu import CASES as HAND, _case

pytestmark = pytest.mark.gpu

KNOBS = ("MXG_GRAPH_RANK", "MXG_GRAPH_U", "MXG_PJ_TWO_LEVEL", "MXG_GRAPH_JOIN", "MXG_DEBUG_JOIN")
GRAPH_KEYS = ("vertex_hash", "vertex_pos", "vertex_record", "edge_u", "edge_v", "edge_support", "edge_weight")


def _keys(rng, n):
    """n distinct 64-bit keys"""
    out = np.unique(rng.integers(1, 2**63, size=n + 64, dtype=np.int64).astype(np.uint64))
    assert out.size >= n
    rng.shuffle(out)
    return out[:n]


def _sets(fv, frec, seed, extra=None):
    """minimizer lists of the filtered lists fv / frec (vertex v = the v-th shared key); extra[a] minimizers that only assembly a
    has are put in between, each in the record of the entry it lands in front of"""
    rng = np.random.default_rng(seed)
    nv = fv[0].size
    extra = extra or [0] * len(fv)
    keys = _keys(rng, nv + sum(extra))
    shared, at, sets = keys[:nv], nv, []
    for a in range(len(fv)):
        hs, rec = shared[fv[a]].tolist(), frec[a].tolist()
        for k in keys[at:at + extra[a]].tolist():
            i = int(rng.integers(0, len(hs) + 1))
            rec.insert(i, rec[i] if i < len(rec) else (rec[-1] if rec else 0))
            hs.insert(i, k)
        at += extra[a]
        hs, rec = np.array(hs, dtype=np.uint64), np.array(rec, dtype=np.uint32)
        sets.append((hs, np.arange(hs.size, dtype=np.uint32) * 3 + a, rec, [f"c{i}" for i in range(int(rec.max()) + 1 if rec.size else 1)]))
    return sets


def _lists(A, nv, seed, longest=40):
    """filtered lists of A assemblies over nv vertices: assembly 0 in order, cut into records of 1 .. longest; every other one a
    random mix of assembly 0's records kept, reversed and shuffled, in shuffled order, cut into records of its own"""
    rng = np.random.default_rng(seed)

    def cut(order):
        recs, at = [], 0
        while at < len(order):
            n = int(rng.integers(1, longest + 1))
            recs.append(order[at:at + n])
            at += n
        return recs

    first = cut(list(range(nv)))
    lists = [first]
    for _ in range(1, A):
        chunks = [list(ch) for ch in first]
        rng.shuffle(chunks)
        order = []
        for ch in chunks:
            how = int(rng.integers(0, 3))
            order += ch if how == 0 else ch[::-1] if how == 1 else rng.permutation(ch).tolist()
        lists.append(cut(order))
    return lists


def _arrays(lists):
    if not lists[0] or not lists[0][0]:
        return [np.zeros(0, np.int64) for _ in lists], [np.zeros(0, np.int64) for _ in lists]
    return _case(lists)


def _cases():
    c = {}
    for name in ("one assembly, three records", "two assemblies by hand", "one vertex", "two vertices, two records"):
        c[name] = (_sets(*_case(HAND[name]), seed=1), {})
    # the vertex count below the rows' stride: one assembly has minimizers of its own (and then both)
    c["nv below the stride"] = (_sets(*_case(HAND["two assemblies by hand"]), seed=2, extra=[0, 5]), {})
    c["nv below the stride, 300"] = (_sets(*_arrays(_lists(2, 300, 3)), seed=3, extra=[40, 7]), {})
    # vertex counts around a 256-block, a thread block of two and of four, at every width of the passes
    for nv in (0, 1, 2, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025):
        sets = _sets(*_arrays(_lists(2, nv, 100 + nv)), seed=100 + nv, extra=[3, 9])
        for u in ("1", "2", "4"):
            c[f"nv{nv} U{u}"] = (sets, {"MXG_GRAPH_U": u})
    # rows far longer than the vertex count (the stride is the smallest assembly's size): whole 256-blocks and whole thread blocks
    # of items beyond the count, which the rank kernels leave without reading -- in the middle (row 0's tail) and at the end,
    # where the last tile still has to report the totals; nv0: every block
    for nv in (0, 1, 300, 1025):
        sets = _sets(*_arrays(_lists(2, nv, 300 + nv)), seed=300 + nv, extra=[1400, 1300])
        for u in ("1", "2", "4"):
            c[f"nv{nv} stride+1300 U{u}"] = (sets, {"MXG_GRAPH_U": u})
    c["A4 stride+2100"] = (_sets(*_arrays(_lists(4, 500, 41)), seed=41, extra=[2100, 2300, 2200, 2500]), {"MXG_GRAPH_U": "4"})
    c["A9 stride+1100"] = (_sets(*_arrays(_lists(9, 200, 42)), seed=42, extra=[1100 + 10 * a for a in range(9)]), {"MXG_GRAPH_U": "2"})
    # every mask form: the places requested up front (A <= 4), the flag byte as the mask (A <= 8), the mask looked up again
    for A in (3, 4, 5, 8, 9, 32):
        c[f"A{A}"] = (_sets(*_arrays(_lists(A, 300, 200 + A, longest=12)), seed=200 + A, extra=[(5 * a) % 7 for a in range(A)]), {})
    c["A3 width 4"] = (_sets(*_arrays(_lists(3, 1100, 77)), seed=77, extra=[1, 0, 2]), {"MXG_GRAPH_U": "4"})
    c["fuzz A3"] = (_sets(*_arrays(_lists(3, 2000, 9)), seed=9, extra=[11, 0, 30]), {})
    return c


CASES = _cases()


def _join_lines(err):
    return [dict((k, int(v)) for k, v in re.findall(r"(\w+)=(\d+)", ln)) for ln in err.splitlines() if ln.startswith("[mxg] join")]


def _env(monkeypatch, env):
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    for key, val in dict(env, MXG_DEBUG_JOIN="1").items():
        monkeypatch.setenv(key, val)


def _build(monkeypatch, capfd, sets, env):
    """-> (the graph, the [mxg] join lines of the build)"""
    from ntjoin_amd.engine import MxEngine
    _env(monkeypatch, env)
    with MxEngine(k=32, w=1000) as eng:
        for a, (hs, pos, rec, ids) in enumerate(sets):
            eng.add_minimizers(f"a{a}", 1.0 + a / 4, hs, pos, rec, ids)
        eng.build_graph()
        capfd.readouterr()
        eng.build_graph()  # twice on one handle: the second build finds the first one's places and counts in its arrays
        lines = _join_lines(capfd.readouterr().err)
        g = eng.get_graph()
        return {key: np.asarray(g[key]).copy() for key in GRAPH_KEYS}, lines


def _oracle_edges(hashes, recs, weights):
    g = _oracle.load().graph(hashes, recs, weights, edges=True)
    return g["vertices"], sorted(zip(g["eu"].tolist(), g["ev"].tolist(), g["esup"].tolist(), g["ew"].tolist()))


def _edges_by_hash(g):
    vh = g["vertex_hash"]
    return sorted(zip(vh[g["edge_u"]].tolist(), vh[g["edge_v"]].tolist(), g["edge_support"].tolist(), g["edge_weight"].tolist()))


def _both_routes_equal_the_oracle(build, reference):
    """build(route) -> (graph, join lines); reference() -> (vertex count, edges by hash) of the C oracle"""
    got = {}
    for route in ("1", "0"):
        got[route], lines = build(route)
        assert len(lines) == 1, lines
        assert lines[0]["pj"] == 1 and lines[0]["rank"] == int(route), lines
    for key in GRAPH_KEYS:
        assert np.array_equal(got["1"][key], got["0"][key]), key
    n_vertices, edges = reference()
    assert len(got["1"]["vertex_hash"]) == n_vertices
    assert _edges_by_hash(got["1"]) == edges
    return got["1"]


@pytest.mark.parametrize("name", list(CASES))
def test_rank_route_equals_table_route_and_oracle(name, monkeypatch, capfd):
    sets, env = CASES[name]
    g = _both_routes_equal_the_oracle(lambda route: _build(monkeypatch, capfd, sets, dict(env, MXG_GRAPH_RANK=route)),
                                      lambda: _oracle_edges([s[0] for s in sets], [s[2] for s in sets], [1.0 + a / 4 for a in range(len(sets))]))
    for a, s in enumerate(sets):  # every vertex sits where its key does in every assembly
        where = {int(h): i for i, h in enumerate(s[0].tolist())}
        idx = np.array([where[int(h)] for h in g["vertex_hash"].tolist()], dtype=np.int64)
        assert np.array_equal(g["vertex_pos"][a], s[1][idx]) and np.array_equal(g["vertex_record"][a], s[2][idx]), a


def test_hand_case_has_the_edges_it_was_made_for(monkeypatch, capfd):
    """the pairs the hand case is about, by vertex: (1, 2) supported by both assemblies although assembly 1 lists it in reverse;
    (3, 4) by assembly 0 alone although their places in assembly 1 differ by one (two records); (6, 7) by assembly 1 alone
    although their places in assembly 0 differ by one (two records); nothing leaves the one-vertex record's row end"""
    sets, env = CASES["two assemblies by hand"]
    g, _ = _build(monkeypatch, capfd, sets, dict(env, MXG_GRAPH_RANK="1"))
    sup = {(int(u), int(v)): int(m) for u, v, m in zip(g["edge_u"], g["edge_v"], g["edge_support"])}
    sup.update({(v, u): m for (u, v), m in list(sup.items())})
    assert sup[(1, 2)] == 3 and sup[(0, 1)] == 3
    assert sup[(3, 4)] == 1 and sup[(4, 5)] == 1
    assert sup[(6, 7)] == 2 and sup[(5, 3)] == 2 and sup[(4, 6)] == 2
    assert len(g["edge_u"]) == 8 and (2, 3) in sup and (5, 6) not in sup


def test_fused_call_on_both_routes(monkeypatch, capfd):
    """sketch_graph() on a 2 x 1 Mbp synthetic pair: the vertex count is still on the device when the edge passes run"""
    import torch
    from ntjoin_amd import synth
    from ntjoin_amd.engine import MxEngine
    ref, tgt = synth.config2(seed=7, n_bases=1_000_000)
    sketches = {}

    def build(route):
        _env(monkeypatch, {"MXG_GRAPH_RANK": route})
        with MxEngine(k=32, w=1000) as eng:
            for name, wt, recs in (("ref", 2.0, ref), ("tgt", 1.0, tgt)):
                words, starts, lens = synth.pack_records(recs)
                d = torch.from_numpy(words.view(np.int32)).cuda()
                eng.add_packed_device(name, wt, d.data_ptr(), starts, lens, keepalive=d)
            capfd.readouterr()
            eng.sketch_graph()
            lines = _join_lines(capfd.readouterr().err)
            for a in range(2):
                sk = eng.get_sketch(a)
                sketches[a] = (sk["out_hash"].copy(), sk["record"].copy())
            g = eng.get_graph()
            return {key: np.asarray(g[key]).copy() for key in GRAPH_KEYS}, lines

    def reference():
        nv, edges = _oracle_edges([sketches[a][0] for a in range(2)], [sketches[a][1] for a in range(2)], [2.0, 1.0])
        assert nv > 500 and len(edges) > 500
        return nv, edges

    _both_routes_equal_the_oracle(build, reference)
