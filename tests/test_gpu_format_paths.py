"""GPU tests of the path stage in one call (mxg_format_paths / MxEngine.format_paths / Ntjoin.format_paths): nodes, orientations
and gap sizes of all paths against (1) the reference's own format_path rows committed in the goldens, (2) constructed shapes with
the expected values written out, (3) Ntjoin._format_paths_host (the host loop the call replaces) on random three-assembly
inputs, plus the errors, the order of calls and the Python face."""
import argparse
import contextlib
import io
import os
import random
import types

import numpy as np
import pytest

from tests._format_cases import _random_assemblies
from tests.conftest import GOLDEN, golden_cases, load_case

pytestmark = pytest.mark.gpu

CASES = [m["name"] for m in golden_cases()]
K = 32
NODE_U32 = ("record", "start", "end", "contig_size", "first_vertex", "terminal_vertex", "segment")


def _fasta_lengths(path):
    lens, rid = {}, None
    for line in open(path, encoding="ascii"):
        if line.startswith(">"):
            rid = line[1:].split()[0]
            lens[rid] = 0
        elif rid is not None:
            lens[rid] += len(line.strip())
    return lens


def _rows(eng, a, nodes):
    "the rows of format_path from the arrays of MxEngine.format_paths, through record_ids / vertex_hash: one list per path"
    ids = eng.record_ids(a, eng.n_records(a))
    vh = eng.get_graph()["vertex_hash"]
    nf = nodes["node_first"].tolist()
    assert nf[0] == 0 and nf[-1] == len(nodes["record"]) and all(x <= y for x, y in zip(nf, nf[1:]))
    for name in NODE_U32 + ("reverse", "gap_size", "raw_gap_size"):
        assert len(nodes[name]) == nf[-1], name
    rows = [[ids[r], "-" if rv else "+", s, e, c, str(int(vh[f])), str(int(vh[t])), g, rg] for r, rv, s, e, c, f, t, g, rg in
            zip(*[nodes[c].tolist() for c in ("record", "reverse", "start", "end", "contig_size", "first_vertex",
                                              "terminal_vertex", "gap_size", "raw_gap_size")])]
    return [rows[lo:hi] for lo, hi in zip(nf, nf[1:])]


def _check_segments(eng, a, nodes):
    "segment[i] is a run of path_segments with the node's record, runs ascend, and the path of the run is the node's path"
    seg = eng.path_segments(a)
    sg = nodes["segment"]
    assert np.all(sg[1:] > sg[:-1])
    assert np.array_equal(seg["record"][sg], nodes["record"])
    nf = nodes["node_first"]
    path_of_node = np.searchsorted(nf, np.arange(len(sg)), side="right") - 1
    assert np.array_equal(seg["path"][sg].astype(np.int64), path_of_node)
    return seg


class _Host:
    "Ntjoin around an engine that was loaded by hand: what _format_paths_host and format_paths read of it"

    def __init__(self, eng, order, found):
        from ntjoin_amd.ntjoin import Ntjoin
        nj = self.nj = Ntjoin.__new__(Ntjoin)
        nj.args = argparse.Namespace(k=K)
        nj._engine, nj._order, nj._found = eng, list(order), found
        names = [str(h) for h in eng.get_graph()["vertex_hash"].tolist()]
        nj._graph, nj._graph_pending = types.SimpleNamespace(names=names), False


def _against_host(eng, order, found, lengths, **kw):
    """MxEngine.format_paths and Ntjoin.format_paths against Ntjoin._format_paths_host on the same handle (target = the last
    assembly); returns (the arrays, the rows)"""
    tgt = len(order) - 1
    ids = eng.record_ids(tgt, eng.n_records(tgt))
    host = _Host(eng, order, found)
    want = host.nj._format_paths_host(lengths, kw.get("g", 20), kw.get("G", 0), kw.get("m", 90), kw.get("mkt", False))
    nodes = eng.format_paths(tgt, lengths=[lengths[c] for c in ids], **kw)
    got = _rows(eng, tgt, nodes)
    assert got == want
    assert host.nj.format_paths(lengths, kw.get("g", 20), kw.get("G", 0), kw.get("m", 90), kw.get("mkt", False)) == want
    assert int(nodes["node_first"][-1]) == sum(len(p) for p in want) and len(nodes["node_first"]) == len(found) + 1
    _check_segments(eng, tgt, nodes)
    return nodes, got


# ---- 1. goldens ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_format_paths_match_reference_goldens(name):
    """every golden case at every -n: the rows built from MxEngine.format_paths equal the reference's format_path rows"""
    from ntjoin_amd.engine import MxEngine
    case = load_case(name)
    meta, ref = case["meta"], case["reference"]
    fa = ref["format_args"]
    lengths = _fasta_lengths(os.path.join(GOLDEN, "fasta", meta["target"]["fasta"]))
    cdir = os.path.join(GOLDEN, "cases", name)
    asms = meta["refs"] + [meta["target"]]
    tgt = len(asms) - 1
    with MxEngine(k=meta["k"], w=meta["w"], variant=meta["variant"]) as eng:
        for a in asms:
            eng.add_tsv(a["tsv"], a["weight"], os.path.join(cdir, a["tsv"]))
        eng.build_graph()
        ids = eng.record_ids(tgt, eng.n_records(tgt))
        for n, want in ref["format_by_n"].items():
            found = eng.find_paths(int(n))
            nodes = eng.format_paths(tgt, g=fa["g"], G=fa["G"], m=fa["m"], lengths=[lengths[c] for c in ids])
            assert len(nodes["node_first"]) == len(found) + 1
            got = _rows(eng, tgt, nodes)
            key = lambda path: tuple(tuple(x) for x in path)  # noqa: E731
            assert sorted(map(key, got)) == sorted(map(key, want)), (name, n)
            _check_segments(eng, tgt, nodes)


# ---- 2. constructed shapes ----------------------------------------------------------------------------------------------
def _add(eng, name, weight, records):
    "records = [(id, [(hash, pos), ...])]: one assembly through add_minimizers, sorted by (record, position)"
    hs, ps, rs = [], [], []
    for r, (_rid, mxs) in enumerate(records):
        for h, p in sorted(mxs, key=lambda hp: hp[1]):
            hs.append(h)
            ps.append(p)
            rs.append(r)
    eng.add_minimizers(name, weight, np.array(hs, dtype=np.uint64), np.array(ps, dtype=np.uint32), np.array(rs, dtype=np.uint32),
                       [rid for rid, _ in records])


def _h(i):
    return 1_000_003 * (i + 1)


def _shuffled(n, seed):
    "a permutation of n positions that the m rule leaves without an orientation at every m > 60"
    rng = random.Random(seed)
    while True:
        perm = list(range(n))
        rng.shuffle(perm)
        inc = sum(a < b for a, b in zip(perm, perm[1:]))
        if 0.4 * (n - 1) <= inc <= 0.6 * (n - 1):
            return perm


def _abc(eng, n_b, perm_b, len_a=1000, second_ref_break=None):
    """reference r (weight 2): one record of 5 + n_b + 5 minimizers 1000 apart.  Target (weight 1): A = the first five at
    100..500, B = the n_b in the middle at shuffled positions, C = the last five at 100..500.  second_ref_break = i: a second
    reference (weight 2, positions 2000 apart) holds the same minimizers in two records, cut between B's minimizers i - 1 and i,
    so that one edge deep inside the stretch is supported by the first reference alone."""
    n = 10 + n_b
    _add(eng, "r", 2.0, [("chr", [(_h(i), 1000 * i) for i in range(n)])])
    order = ["r"]
    if second_ref_break is not None:
        cut = 5 + second_ref_break
        _add(eng, "r2", 2.0, [("chrA", [(_h(i), 2000 * i) for i in range(cut)]), ("chrB", [(_h(i), 2000 * i) for i in range(cut, n)])])
        order.append("r2")
    _add(eng, "t", 1.0, [("A", [(_h(i), 100 * (i + 1)) for i in range(5)]),
                         ("B", [(_h(5 + i), 10 * (perm_b[i] + 1)) for i in range(n_b)]),
                         ("C", [(_h(5 + n_b + i), 100 * (i + 1)) for i in range(5)])])
    order.append("t")
    eng.build_graph()
    return order, {"A": len_a, "B": 10 * n_b + 100, "C": 1000}


def test_shape_a_junction_spans_an_unoriented_contig():
    """A(+) B(?) C(+) on one path: the junction A -> C spans B's edges; only the reference supports them.
    mean = 6000 - 32; a = 1000 - 500 - 32 = 468; b = 100 - 0; raw = 5968 - 568 = 5400"""
    from ntjoin_amd.engine import MxEngine
    with MxEngine(k=K, w=10) as eng:
        order, lengths = _abc(eng, 5, [3, 1, 4, 0, 2])
        found = eng.find_paths(2)
        assert len(found) == 1 and len(found[0][1]) == 15
        nodes, rows = _against_host(eng, order, found, lengths)
        assert rows == [[["A", "+", 0, 1000, 1000, str(_h(0)), str(_h(4)), 5400, 5400],
                         ["C", "+", 0, 1000, 1000, str(_h(10)), str(_h(14)), 0, 0]]]
        assert nodes["segment"].tolist() == [0, 2] and nodes["node_first"].tolist() == [0, 2]
        # (d) the cap: raw above G gives G and leaves raw; G = 0 leaves the gap uncapped (above)
        nodes, rows = _against_host(eng, order, found, lengths, G=40)
        assert (rows[0][0][7], rows[0][0][8]) == (40, 5400)
        nodes, rows = _against_host(eng, order, found, lengths, g=7000, G=0)
        assert (rows[0][0][7], rows[0][0][8]) == (7000, 5400)


def test_shape_d_negative_raw_gap():
    """A is 7000 bases long and its last minimizer sits at 500: a = 7000 - 500 - 32 = 6468 > mean, raw = 5968 - 6468 - 100 < 0"""
    from ntjoin_amd.engine import MxEngine
    with MxEngine(k=K, w=10) as eng:
        order, lengths = _abc(eng, 5, [3, 1, 4, 0, 2], len_a=7000)
        found = eng.find_paths(2)
        for kw in ({}, {"G": 40}, {"g": 1}):
            _nodes, rows = _against_host(eng, order, found, lengths, **kw)
            assert (rows[0][0][7], rows[0][0][8]) == (kw.get("g", 20), -600) and rows[0][0][3] == 7000


@pytest.mark.parametrize("n_b,brk", [(300, 290), (65, 64)])
def test_shape_b_long_stretch(n_b, brk):
    """B of n_b minimizers: the stretch A -> C is n_b + 1 edges (beyond 64 and beyond 256 lanes).  Every edge is supported by both
    references but edge number brk of the stretch (the second reference is cut there), so common = the first reference alone:
    mean = 1000 (n_b + 1) - 32 whereas both references would give 1500 (n_b + 1) - 32; raw = mean - 468 - 100"""
    from ntjoin_amd.engine import MxEngine
    with MxEngine(k=K, w=10) as eng:
        order, lengths = _abc(eng, n_b, _shuffled(n_b, n_b), second_ref_break=brk)
        found = eng.find_paths(2)
        assert len(found) == 1 and len(found[0][1]) == n_b + 10
        nodes, rows = _against_host(eng, order, found, lengths)
        raw = 1000 * (n_b + 1) - 32 - 468 - 100
        assert rows == [[["A", "+", 0, 1000, 1000, str(_h(0)), str(_h(4)), raw, raw],
                         ["C", "+", 0, 1000, 1000, str(_h(n_b + 5)), str(_h(n_b + 9)), 0, 0]]]
        seg = eng.path_segments(len(order) - 1)
        s0, s1 = nodes["segment"].tolist()
        assert int(seg["first"][s1]) - (int(seg["first"][s0]) + int(seg["n"][s0]) - 1) == n_b + 1
        # the edge the second reference lacks is edge number brk of the stretch
        g = eng.get_graph()
        masks = {frozenset(e): s for e, s in zip(zip(g["edge_u"].tolist(), g["edge_v"].tolist()), g["edge_support"].tolist())}
        verts = found[0][1]
        stretch = [masks[frozenset(e)] & 3 for e in zip(verts[4:n_b + 5], verts[5:n_b + 6])]
        assert [i for i, s in enumerate(stretch) if s != 3] == [brk] and stretch[brk] == 1


def test_shape_c_empty_common_support():
    """three assemblies of weight 1: the stretch u - x - v (x: a target contig of one minimizer, no orientation) has its first
    edge from the first reference only and its second from the second only: the AND is empty, gap = raw = g"""
    from ntjoin_amd.engine import MxEngine
    a0, a1, u, x, v, c1, c2 = (_h(i) for i in range(7))
    with MxEngine(k=K, w=10) as eng:
        _add(eng, "r1", 1.0, [("p", [(a0, 1000), (a1, 2000), (u, 3000), (x, 4000)]), ("q", [(v, 1000), (c1, 2000), (c2, 3000)])])
        _add(eng, "r2", 1.0, [("p", [(a0, 1000), (a1, 2000), (u, 3000)]), ("q", [(x, 500), (v, 1000), (c1, 2000), (c2, 3000)])])
        _add(eng, "t", 1.0, [("A", [(a0, 100), (a1, 200), (u, 300)]), ("X", [(x, 50)]), ("C", [(v, 1100), (c1, 1200), (c2, 1300)])])
        order, lengths = ["r1", "r2", "t"], {"A": 400, "X": 100, "C": 2000}
        eng.build_graph()
        found = eng.find_paths(1)
        assert len(found) == 1 and len(found[0][1]) == 7
        g = eng.get_graph()
        vh = g["vertex_hash"].tolist()
        masks = {frozenset((vh[a], vh[b])): s for a, b, s in zip(g["edge_u"].tolist(), g["edge_v"].tolist(), g["edge_support"].tolist())}
        assert masks[frozenset((u, x))] == 1 and masks[frozenset((x, v))] == 2 and masks[frozenset((u, x))] & masks[frozenset((x, v))] == 0
        for gmin in (20, 3):
            _nodes, rows = _against_host(eng, order, found, lengths, g=gmin)
            assert rows == [[["A", "+", 0, 400, 400, str(a0), str(u), gmin, gmin], ["C", "+", 0, 2000, 2000, str(v), str(c2), 0, 0]]]


def test_shape_e_empty_path_single_node_and_reverse_pair():
    """three paths: P (four target contigs of one minimizer each: no node), Q (one oriented run and a single minimizer: one node,
    gap 0, 0), S (D and E both decreasing: a = 100 - 0, b = 1000 - 300 - 32 = 668, raw = 968 - 768 = 200)"""
    from ntjoin_amd.engine import MxEngine
    P, Q, S = [_h(i) for i in range(4)], [_h(10 + i) for i in range(4)], [_h(20 + i) for i in range(6)]
    with MxEngine(k=K, w=10) as eng:
        _add(eng, "r", 2.0, [(nm, [(h, 1000 * (i + 1)) for i, h in enumerate(hs)]) for nm, hs in (("rp", P), ("rq", Q), ("rs", S))])
        tgt = [(f"P{i}", [(h, 77)]) for i, h in enumerate(P)]
        tgt += [("Q", [(h, 100 * (i + 1)) for i, h in enumerate(Q[:3])]), ("Q3", [(Q[3], 5)])]
        tgt += [("D", [(h, 300 - 100 * i) for i, h in enumerate(S[:3])]), ("E", [(h, 300 - 100 * i) for i, h in enumerate(S[3:])])]
        _add(eng, "t", 1.0, tgt)
        lengths = {rid: 1000 for rid, _ in tgt}
        eng.build_graph()
        found = eng.find_paths(2)
        assert sorted(len(p) for _c, p in found) == [4, 4, 6]
        nodes, rows = _against_host(eng, ["r", "t"], found, lengths)
        assert len(nodes["node_first"]) == 4
        by_len = {len(p): r for (_c, p), r in zip(found, rows)}
        assert sorted(map(len, rows)) == [0, 1, 2]
        assert [r for r in rows if len(r) == 1] == [[["Q", "+", 0, 1000, 1000, str(Q[0]), str(Q[2]), 0, 0]]]
        assert by_len[6] == [["D", "-", 0, 1000, 1000, str(S[0]), str(S[2]), 200, 200],
                             ["E", "-", 0, 1000, 1000, str(S[3]), str(S[5]), 0, 0]]


def test_shape_f_m_rule_boundary_and_mkt():
    """U: 11 minimizers with 9 of 10 pairs increasing: 9 / 10 * 100 == 90 exactly, '+' at m = 90.  W: 5 minimizers with 3 of 4
    pairs increasing: 75 %, '?' at m = 90 and '+' at m = 75.  With mkt the statistics decide both."""
    from ntjoin_amd.engine import MxEngine
    from ntjoin_amd.ntjoin import Ntjoin, mk_orientation
    from tests.test_mkt_cpu import _s_ties
    u_pos = [100, 200, 300, 400, 500, 700, 600, 800, 900, 1000, 1100]
    w_pos = [100, 200, 400, 300, 500]
    assert 9 / float(10) * 100 == 90 and Ntjoin.determine_orientation(11, 9, 1, 90) == "+"
    assert Ntjoin.determine_orientation(5, 3, 1, 90) == "?" and Ntjoin.determine_orientation(5, 3, 1, 75) == "+"
    U, W = [_h(i) for i in range(11)], [_h(11 + i) for i in range(5)]
    with MxEngine(k=K, w=10) as eng:
        _add(eng, "r", 2.0, [("chr", [(h, 1000 * (i + 1)) for i, h in enumerate(U + W)])])
        _add(eng, "t", 1.0, [("U", list(zip(U, u_pos))), ("W", list(zip(W, w_pos)))])
        lengths = {"U": 2000, "W": 2000}
        eng.build_graph()
        found = eng.find_paths(2)
        assert len(found) == 1 and len(found[0][1]) == 16
        _n, rows = _against_host(eng, ["r", "t"], found, lengths, m=90)
        assert [(r[0], r[1]) for r in rows[0]] == [("U", "+")]
        _n, rows = _against_host(eng, ["r", "t"], found, lengths, m=75)
        # u = U's last path vertex (target position 1100), v = W's first (100): mean = 1000 - 32, a = 2000 - 1100 - 32, b = 100
        assert rows == [[["U", "+", 0, 2000, 2000, str(U[0]), str(U[10]), 20, 968 - 868 - 100],
                         ["W", "+", 0, 2000, 2000, str(W[0]), str(W[4]), 0, 0]]]
        want = [mk_orientation(len(x), *_s_ties(x)) for x in (u_pos, w_pos)]
        assert want == ["+", "?"]
        _n, rows = _against_host(eng, ["r", "t"], found, lengths, m=75, mkt=True)
        assert [(r[0], r[1]) for r in rows[0]] == [("U", "+")]


class _Swapped:
    "an engine seen with assemblies 0 and t exchanged: _format_paths_host, which formats the last assembly, then formats assembly 0"

    def __init__(self, eng, t):
        self._eng, self._t = eng, t

    def _a(self, a):
        return {0: self._t, self._t: 0}.get(a, a)

    def record_ids(self, a, n):
        return self._eng.record_ids(self._a(a), n)

    def n_records(self, a):
        return self._eng.n_records(self._a(a))

    def mx_extremes(self, a):
        return self._eng.mx_extremes(self._a(a))

    def path_segments(self, a):
        return self._eng.path_segments(self._a(a))

    def path_segments_mk(self, a):
        return self._eng.path_segments_mk(self._a(a))

    def get_graph(self):
        g = dict(self._eng.get_graph())
        t = self._t
        vp = g["vertex_pos"].copy()
        vp[[0, t]] = vp[[t, 0]]
        s = g["edge_support"].astype(np.int64)
        b0, bt = s & 1, s >> t & 1
        g["vertex_pos"], g["edge_support"] = vp, (s & ~(1 | 1 << t)) | bt | b0 << t
        return g


def test_shape_g_a_reference_as_the_formatted_assembly():
    """assembly = 0 (the second reference of shape (b), two records, orientation '+'): against the host route on the same
    handle seen with assemblies 0 and 2 exchanged.  chrA holds minimizers 0..68 at 2000 i, chrB 69..74 from 40 on: the junction
    is one edge supported by r alone (r2 is cut there): mean = 1000 - 32, a = 136100 - 136000 - 32 = 68, b = 40 - 0"""
    from ntjoin_amd.engine import MxEngine
    with MxEngine(k=K, w=10) as eng:
        n_b, brk = 65, 64
        n = 10 + n_b
        _add(eng, "r2", 2.0, [("chrA", [(_h(i), 2000 * i) for i in range(5 + brk)]), ("chrB", [(_h(i), 2000 * (i - 5 - brk) + 40) for i in range(5 + brk, n)])])
        _add(eng, "r", 2.0, [("chr", [(_h(i), 1000 * i) for i in range(n)])])
        perm = _shuffled(n_b, n_b)
        _add(eng, "t", 1.0, [("A", [(_h(i), 100 * (i + 1)) for i in range(5)]), ("B", [(_h(5 + i), 10 * (perm[i] + 1)) for i in range(n_b)]),
                             ("C", [(_h(5 + n_b + i), 100 * (i + 1)) for i in range(5)])])
        eng.build_graph()
        found = eng.find_paths(2)
        assert len(found) == 1
        g = eng.get_graph()
        vh = g["vertex_hash"].tolist()
        cut = {frozenset((vh[a], vh[b])): s for a, b, s in zip(g["edge_u"].tolist(), g["edge_v"].tolist(), g["edge_support"].tolist())}
        assert cut[frozenset((_h(68), _h(69)))] == 2   # r alone
        lengths = {"chrA": 136_100, "chrB": 150_000}
        host = _Host(eng, ["r2", "r", "t"], found)
        host.nj._engine = _Swapped(eng, 2)
        want = host.nj._format_paths_host(lengths)
        nodes = eng.format_paths(0, lengths=[lengths["chrA"], lengths["chrB"]])
        assert _rows(eng, 0, nodes) == want
        assert want == [[["chrA", "+", 0, 136_100, 136_100, str(_h(0)), str(_h(68)), 968 - 68 - 40, 968 - 68 - 40],
                         ["chrB", "+", 0, 150_000, 150_000, str(_h(69)), str(_h(74)), 0, 0]]]
        _check_segments(eng, 0, nodes)


# ---- 3. fuzz (the generator: tests/_format_cases.py) --------------------------------------------------------------------
def test_fuzz_against_host_route():
    """random three-assembly inputs; m in {50, 75, 90}, g in {1, 20}, G in {0, 40}, mkt on and off; every field against
    _format_paths_host.  The four kinds of case the kernels treat differently are counted and each must occur.
    Seed 20, 12 trials, one parameter set per trial; a plain walk over the paths of oracle/paths_oracle.py on the same inputs
    (no GPU) counts 27 paths, 34 junctions with a stretch of more than one edge, 1 with empty support, 17 G-capped junctions in
    the trials without mkt (format_path of the oracle has no mkt) and 18 runs decided by the Mann-Kendall branch."""
    from ntjoin_amd.engine import MxEngine
    rng = random.Random(20)
    long_stretch = empty_support = capped = mk_runs = n_paths = 0
    for trial in range(12):
        asms, lengths = _random_assemblies(rng)
        weights = rng.choice([(1.0, 1.0, 1.0), (2.0, 1.0, 1.0), (1.0, 2.0, 1.0), (2.0, 2.0, 1.0)])
        m, g, G, mkt = (50, 75, 90)[trial % 3], (1, 20)[trial // 3 % 2], (0, 40)[trial // 6 % 2], trial % 2 == 1
        with MxEngine(k=K, w=10) as eng:
            order = ["r0", "r1", "t"]
            for nm, wt, recs in zip(order, weights, asms):
                _add(eng, nm, wt, recs)
            eng.build_graph()
            found = eng.find_paths(1 if trial % 4 else 2)
            nodes, _rws = _against_host(eng, order, found, lengths, m=m, g=g, G=G, mkt=mkt)
            n_paths += len(found)
            # what kind of cases this was: a plain walk over the runs and the graph's masks
            seg = eng.path_segments(2)
            gr = eng.get_graph()
            masks = {frozenset(e): s for e, s in zip(zip(gr["edge_u"].tolist(), gr["edge_v"].tolist()), gr["edge_support"].tolist())}
            flat = [v for _c, p in found for v in p]
            nf, sg = nodes["node_first"].tolist(), nodes["segment"].tolist()
            for lo, hi in zip(nf, nf[1:]):
                for j in range(lo, hi - 1):
                    iu, iv = int(seg["first"][sg[j]]) + int(seg["n"][sg[j]]) - 1, int(seg["first"][sg[j + 1]])
                    long_stretch += iv - iu > 1
                    common = -1
                    for e in zip(flat[iu:iv], flat[iu + 1:iv + 1]):
                        common &= masks[frozenset(e)]
                    empty_support += common == 0
                    if common == 0:
                        assert int(nodes["gap_size"][j]) == int(nodes["raw_gap_size"][j]) == g
                    capped += G > 0 and int(nodes["raw_gap_size"][j]) > G and int(nodes["gap_size"][j]) == G
            if mkt:
                mk_runs += int(np.sum((seg["n"] > 1) & (seg["inc"] != seg["n"] - 1) & (seg["dec"] != seg["n"] - 1)))
    print("fuzz counts:", dict(paths=n_paths, long_stretch=long_stretch, empty_support=empty_support, capped=capped, mk_runs=mk_runs))
    assert long_stretch > 0 and empty_support > 0 and capped > 0 and mk_runs > 0


# ---- 4. errors and order of calls ---------------------------------------------------------------------------------------
def test_errors_and_order_of_calls(tmp_path):
    from ntjoin_amd import capi
    from ntjoin_amd.engine import MxEngine, MxError
    with MxEngine(k=K, w=10) as eng:
        order, lengths = _abc(eng, 5, [3, 1, 4, 0, 2])
        lens = [lengths[c] for c in "ABC"]
        with pytest.raises(MxError) as ei:   # before find_paths
            eng.format_paths(1, lengths=lens)
        assert ei.value.code == capi.MXG_EINVAL
        found = eng.find_paths(2)
        for a in (2, -1, 99):
            with pytest.raises(MxError) as ei:
                eng.format_paths(a, lengths=lens)
            assert ei.value.code == capi.MXG_EINVAL
        with pytest.raises(MxError) as ei:   # minimizer input holds no lengths
            eng.format_paths(1)
        assert ei.value.code == capi.MXG_EINVAL
        host = _Host(eng, order, found)
        with pytest.raises(ValueError, match="holds no contig lengths"):
            host.nj.format_paths()
        p = capi.FormatParams()
        p.struct_size, p.g, p.m = 16, 20, 90.0
        import ctypes as C
        assert eng._lib.mxg_format_paths(eng._h, 1, C.byref(p), None, C.byref(capi.PathNodesView())) == capi.MXG_EINVAL
        # A's run ends at A's largest position, 500: its end is A's length.  531 = 500 + k - 1 makes the overhang -1
        short = dict(lengths, A=531)
        with pytest.raises(MxError) as ei:
            eng.format_paths(1, lengths=[short[c] for c in "ABC"])
        assert ei.value.code == capi.MXG_EINVAL and "less than 0" in str(ei.value) and "path 0 node 0" in str(ei.value)
        with pytest.raises(ValueError) as ev:
            host.nj.format_paths(short)
        with pytest.raises(ValueError) as eh:
            host.nj._format_paths_host(short)
        assert str(ev.value) == str(eh.value) and str(ev.value).startswith("Gap distance estimation less than 0 between ['A', '+', 0, 531")
        # ... and the handle formats correctly afterwards; the other calls return what they returned before
        seg0, mk0, ext0 = eng.path_segments(1), eng.path_segments_mk(1), eng.mx_extremes(1)
        _nodes, rows = _against_host(eng, order, found, lengths)
        assert rows[0][0][7:] == [5400, 5400]
        seg1, mk1, ext1 = eng.path_segments(1), eng.path_segments_mk(1), eng.mx_extremes(1)
        assert all(np.array_equal(seg0[c], seg1[c]) for c in seg0) and all(np.array_equal(mk0[c], mk1[c]) for c in mk0) and ext0 == ext1
        eng.format_paths(1, lengths=lens, mkt=True)
        mk2 = eng.path_segments_mk(1)   # straight after the call: the runs it left are those of path_segments(1)
        assert all(np.array_equal(mk0[c], mk2[c]) for c in mk0)
        # a contig of some node that lengths does not hold: KeyError, as the host route's lengths[contig]
        for route in (host.nj.format_paths, host.nj._format_paths_host):
            with pytest.raises(KeyError, match="C"):
                route({"A": 1000, "B": 150})
        # the endpoints' hashes, gathered on the device, are those of the graph view
        vh = eng.get_graph()["vertex_hash"]
        idx = np.array([3, 0, 14, 3], dtype=np.uint32)
        assert np.array_equal(eng.vertex_hashes(idx), vh[idx]) and len(eng.vertex_hashes([])) == 0
        with pytest.raises(MxError):
            eng.vertex_hashes([15])
        # a -n no edge reaches: no path, no node
        assert eng.find_paths(100) == []
        nodes = eng.format_paths(1, lengths=lens)
        assert nodes["node_first"].tolist() == [0] and all(len(nodes[c]) == 0 for c in NODE_U32 + ("reverse", "gap_size", "raw_gap_size"))
    # a TSV-loaded target holds no lengths either
    name = "f-f_w1000"
    meta = load_case(name)["meta"]
    cdir = os.path.join(GOLDEN, "cases", name)
    with MxEngine(k=meta["k"], w=meta["w"], variant=meta["variant"]) as eng:
        for a in meta["refs"] + [meta["target"]]:
            eng.add_tsv(a["tsv"], a["weight"], os.path.join(cdir, a["tsv"]))
        eng.build_graph()
        eng.find_paths(1)
        with pytest.raises(MxError) as ei:
            eng.format_paths(len(meta["refs"]))
        assert ei.value.code == capi.MXG_EINVAL


# ---- 5. the Python face -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mkt", [("f-f_w1000", False), ("synth_w100", True)])
def test_ntjoin_format_paths_without_the_graph_object(name, mkt):
    """Ntjoin.format_paths after make_minimizer_graph(materialize=False) makes no graph object (no name per vertex, no edge
    dict) and equals the host route"""
    from ntjoin_amd.ntjoin import Ntjoin
    case = load_case(name)
    meta, fa = case["meta"], case["reference"]["format_args"]
    lengths = _fasta_lengths(os.path.join(GOLDEN, "fasta", meta["target"]["fasta"]))
    cwd = os.getcwd()
    os.chdir(os.path.join(GOLDEN, "cases", name))
    try:
        args = argparse.Namespace(FILES=[r["tsv"] for r in meta["refs"]], s=meta["target"]["tsv"], l=meta["target"]["weight"],
                                  p="/tmp/mxg_fmtnodes_" + name, k=meta["k"], n=1, t=1)
        nj = Ntjoin(args, variant=meta["variant"])
        try:
            nj.weights_list = [r["weight"] for r in meta["refs"]]
            with contextlib.redirect_stdout(io.StringIO()):
                nj.load_minimizers_scaffold()
                nj.make_minimizer_graph(materialize=False)
            nj._found = nj._engine.find_paths(1)   # (Ntjoin.find_paths names every vertex: not this test's subject)
            got = nj.format_paths(lengths, g=fa["g"], G=fa["G"], m=fa["m"], mkt=mkt)   # (no host mirror of the graph yet)
            assert nj._graph is None
            with pytest.raises(ValueError, match="holds no contig lengths"):
                nj.format_paths(g=fa["g"], G=fa["G"], m=fa["m"], mkt=mkt)
            assert nj._graph is None
            want = nj._format_paths_host(lengths, g=fa["g"], G=fa["G"], m=fa["m"], mkt=mkt)
        finally:
            nj.close()
        assert got == want and sum(map(len, got)) > 0
    finally:
        os.chdir(cwd)
