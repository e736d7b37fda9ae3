"""CPU tests of the planned path graphs (tests/_path_graphs.py) and of oracle/paths_oracle.py::find_paths on them: what
the seeded corpus reaches, that the builder's two routes agree, hand-written answers for the small shapes, and that the
bucketed find_paths returns what its predecessor returned.  Nothing here touches the library."""
import collections
import os
import random
from collections import defaultdict, deque

import pytest

from oracle import graph_oracle as go
from oracle import paths_oracle as po
from tests import _path_graphs as pg
from tests.conftest import GOLDEN, golden_cases


def _paths(plan, state, n):
    return po.canonical(po.find_paths(state, n))


def _want(plan, label_paths):
    """canonical form of single-path components given as label lists"""
    return {frozenset({plan.names(p)}) for p in label_paths}


# ---- what the corpus reaches ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus_trace(tmp_path_factory):
    td = tmp_path_factory.mktemp("corpus")
    total, shared_top_rings, biggest = collections.Counter(), 0, 0
    for _t, plan in pg.corpus():
        trace = collections.Counter()
        po.find_paths(plan.state(td), 1, trace)
        if plan.weights.count(max(plan.weights)) >= 2:
            shared_top_rings += trace["ring_opened"]
        total.update(trace)
        biggest = max(biggest, plan.n_vertices)
    return total, shared_top_rings, biggest


def test_corpus_coverage(corpus_trace):
    """the committed seed at n = 1 (DESIGN.md 4b quotes these counters); the generator meets them by the oracle alone"""
    total, shared_top_rings, biggest = corpus_trace
    rounds = {k[1]: v for k, v in total.items() if isinstance(k, tuple)}
    print(dict(total), shared_top_rings, biggest)
    assert sum(v for k, v in rounds.items() if k >= 2) >= 50
    assert sum(v for k, v in rounds.items() if k >= 4) >= 10
    assert total["ring_opened"] >= 20 and shared_top_rings >= 5
    assert total["rejected_same_endpoint"] >= 3
    assert total["accepted"] >= 2000
    assert biggest >= 20000
    # (no component of the corpus stays branched when the loop ends: that takes a branch node whose edges are all shared,
    # which pg.star3 plants)


# ---- the builder ------------------------------------------------------------------------------------------------------
SHAPES = {
    "ring": lambda: pg.ring(7, (1, 2, 2)),
    "rings_and_chains": lambda: pg.rings_and_chains(3, 5, 4, 4),
    "chain": lambda: pg.chain(33, "bit_reversed"),
    "comb": lambda: pg.comb(5, (0.5, 1, 1.5, 3)),
    "ladder": lambda: pg.ladder(3, (1, 2, 3)),
    "star3": pg.star3,
    "mixed_chain": lambda: pg.mixed_chain((0.5, 1.5, 1)),
    "ring_no_path": pg.ring_no_path,
    "tie_ring_min": lambda: pg.tie_cases()["ring_min"][0],
    "tie_endpoints": lambda: pg.tie_cases()["endpoints"][0],
    "perturbed_backbone": lambda: pg.perturbed_backbone(400, random.Random(3), plant_rings=3),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_builder_routes_agree(shape, tmp_path):
    """the arrays for add_minimizers and the TSV files give the same oracle state; every label once per assembly"""
    plan = SHAPES[shape]()
    plan.check()
    by_tsv, by_arrays = plan.state(tmp_path), plan.state_from_arrays()
    assert by_tsv.keys() == by_arrays.keys()
    for key in by_tsv:
        assert by_tsv[key] == by_arrays[key], key
    assert len(by_tsv["vertices"]) == plan.n_vertices       # every label is shared, so every label is a vertex
    for a in range(len(plan.weights)):
        hashes, pos, rec, ids = plan.arrays(a)
        assert sorted(hashes.tolist()) == sorted(plan.hash_of.values())
        assert len(pos) == len(rec) == len(hashes) and int(rec.max()) == len(ids) - 1
    assert all(0 < h < 2 ** 63 for h in plan.hash_of.values())


def test_builder_refuses_a_label_missing_or_twice():
    with pytest.raises(AssertionError):
        pg.Plan([(1, [[0, 1, 2]]), (1, [[0, 1]])])
    with pytest.raises(AssertionError):
        pg.Plan([(1, [[0, 1, 2]]), (1, [[0, 1], [2, 1]])])
    with pytest.raises(AssertionError):
        pg.Plan([(1, [[0, 1, 1]]), (1, [[0, 1]])])


def test_id_orders_are_permutations():
    for kind in pg.ID_ORDERS:
        for L in (1, 2, 33, 1000):
            assert sorted(pg.id_order(L, kind)) == list(range(L)), (kind, L)
    assert pg.id_order(8, "bit_reversed") == [0, 4, 2, 6, 1, 5, 3, 7]
    assert pg.id_order(5, "even_odd") == [0, 2, 4, 1, 3]


# ---- hand-written answers ---------------------------------------------------------------------------------------------
# ring(L, weights): assembly a's record starts at label 0, 1, 2 (L = 3, 4) or 0, 2, 4 (L = 6).  (2, 1): opened and oriented by
# assembly 0.  (1, 2): both by assembly 1.  (1, 1): opened by assembly 0 (0 | L-1), where L-1 comes first in assembly 1.
# (1, 2, 2): opened by assembly 1 (before its start r), where r - 1 comes first in assembly 2.
RING_PATHS = {
    (3, (2, 1)): [0, 1, 2], (3, (1, 2)): [1, 2, 0], (3, (1, 1)): [2, 1, 0], (3, (1, 2, 2)): [0, 2, 1],
    (4, (2, 1)): [0, 1, 2, 3], (4, (1, 2)): [1, 2, 3, 0], (4, (1, 1)): [3, 2, 1, 0], (4, (1, 2, 2)): [0, 3, 2, 1],
    (6, (2, 1)): [0, 1, 2, 3, 4, 5], (6, (1, 2)): [2, 3, 4, 5, 0, 1], (6, (1, 1)): [5, 4, 3, 2, 1, 0],
    (6, (1, 2, 2)): [1, 0, 5, 4, 3, 2],
}


@pytest.mark.parametrize("L,weights", sorted(RING_PATHS))
def test_ring_tables(L, weights, tmp_path):
    plan = pg.ring(L, weights)
    trace = {}
    got = po.canonical(po.find_paths(plan.state(tmp_path), 1, trace))
    assert got == _want(plan, [RING_PATHS[L, weights]])
    assert pg.ring_expected(L, weights) == RING_PATHS[L, weights]
    assert trace == {("rounds", 0): 1, "ring_opened": 1, "accepted": 1}


B4 = [("b", i) for i in range(4)]


@pytest.mark.parametrize("weights,rounds,comb_path", [((1, 2, 3), 3, [("t", 0, 1)] + B4 + [("t", 3, 1)]),
                                                      ((0.5, 1, 1.5, 3), 2, B4)])
def test_ladder_and_comb_tables(weights, rounds, comb_path, tmp_path):
    """n = 1.  (1, 2, 3): round 1 removes nothing, 2 the edges of weight 1, 3 those of weight 2.  (0.5, 1, 1.5, 3): round 1
    removes 0.5, round 2 removes 1 and 1.5.  What is left at a branch node is its pair of heaviest edges.
    The comb's backbone ends have degree 3 under (1, 2, 3): after round 2 they are no branch nodes any more, so round 3 leaves
    them their tooth of weight 2 while it takes those of the inner vertices.  Under (0.5, 1, 1.5, 3) they have degree 4, are
    still branch nodes in round 2 and lose every tooth."""
    top = len(weights) - 1
    plan = pg.ladder(2, weights)
    trace = {}
    got = po.canonical(po.find_paths(plan.state(tmp_path), 1, trace))
    assert got == _want(plan, [[("x", i, top), ("b", i), ("y", i)] for i in range(2)])
    assert trace[("rounds", rounds)] == 2 and trace["accepted"] == 2
    plan = pg.comb(4, weights)
    trace = {}
    got = po.canonical(po.find_paths(plan.state(tmp_path), 1, trace))
    assert got == _want(plan, [comb_path])
    assert trace[("rounds", rounds)] == 1 and trace["accepted"] == 1


@pytest.mark.parametrize("name", sorted(pg.tie_cases()))
def test_tie_tables(name, tmp_path):
    plan, want = pg.tie_cases()[name]
    assert _paths(plan, plan.state(tmp_path), 1) == _want(plan, want)


def test_no_path_tables(tmp_path):
    trace = {}
    assert po.find_paths(pg.ring_no_path().state(tmp_path), 1, trace) == [[]]
    assert trace == {("rounds", 0): 1, "ring_opened": 1, "rejected_same_endpoint": 1}
    for n in (0, 1):
        trace = {}
        assert po.find_paths(pg.star3().state(tmp_path), n, trace) == [[]]
        assert trace == {("rounds", 2 - n): 1, "rejected_branched": 1}


def test_mixed_chain_thresholds(tmp_path):
    """the global filter is strict: an edge of weight exactly n stays (0.5 + 1.5 = 2.0 at n = 2 included)"""
    plan = pg.mixed_chain((0.5, 1.5, 1))
    state = plan.state(tmp_path)
    weight = {frozenset((int(s), int(t))): w for s, t, _sup, w in state["edges"]}
    lab = {str(h): l for l, h in plan.hash_of.items()}
    by_label = {frozenset(lab[str(v)] for v in e): w for e, w in weight.items()}
    assert by_label[frozenset((4, 5))] == 2.0 and by_label[frozenset((0, 1))] == 3.0 and by_label[frozenset((2, 3))] == 2.5
    assert by_label[frozenset((3, 4))] == 1.5
    got = {tuple(lab[v] for v in p) for comp in po.find_paths(state, 2) for p in comp}
    kept = {frozenset(e) for p in got for e in zip(p, p[1:])}
    assert frozenset((4, 5)) in kept and frozenset((3, 4)) not in kept
    assert kept == {e for e, w in by_label.items() if w >= 2}


# ---- the bucketed find_paths against its predecessor ------------------------------------------------------------------
def _find_paths_before(state, n):
    """oracle/paths_oracle.py::find_paths as it was before the edges were bucketed (one scan of all edges per component)"""
    weights = state["weights"]
    vertices = list(state["vertices"])
    edges = [(s, t, w) for s, t, _sup, w in state["edges"]]
    if not n <= min(weights.values()):
        edges = [e for e in edges if not e[2] < n]
    max_w = max(weights.values())
    first_max = [a for a, wt in weights.items() if wt == max_w][0]
    last_max = [a for a, wt in weights.items() if wt == max_w][-1]
    info = state["list_mx_info"]
    out = []
    for comp in po._components(vertices, edges):
        cset = set(comp)
        cedges = [e for e in edges if e[0] in cset]
        min_w, total_w = n, sum(weights.values())
        while True:
            deg = po._degrees(comp, cedges)
            if all(d < 3 for d in deg.values()) or not min_w <= total_w:
                break
            branch = {v for v, d in deg.items() if d > 2}
            cedges = [e for e in cedges if not ((e[0] in branch or e[1] in branch) and e[2] < min_w)]
            min_w += 1
        paths = []
        for sub in po._components(comp, cedges):
            sset = set(sub)
            sedges = [e for e in cedges if e[0] in sset]
            deg = po._degrees(sub, sedges)
            sources = [v for v in sub if deg[v] == 1]
            if not sources:
                if all(d == 2 for d in deg.values()):
                    mv = min(sub, key=lambda v: info[first_max][v][1])
                    nbrs = [t if s == mv else s for s, t, _w in sedges if mv in (s, t)]
                    hn = max(nbrs, key=lambda v: info[first_max][v][1])
                    sedges = [e for e in sedges if {e[0], e[1]} != {mv, hn}]
                    sources = [mv, hn]
            if len(sources) != 2:
                continue
            pos = {v: info[last_max][v][1] for v in sources}
            source = [v for v in sources if pos[v] == min(pos.values())][-1]
            target = [v for v in sources if pos[v] == max(pos.values())][-1]
            adj = defaultdict(list)
            for s, t, _w in sedges:
                adj[s].append(t)
                adj[t].append(s)
            prev, dq = {source: None}, deque([source])
            while dq:
                u = dq.popleft()
                for x in adj[u]:
                    if x not in prev:
                        prev[x] = u
                        dq.append(x)
            if target not in prev:
                continue
            path, u = [], target
            while u is not None:
                path.append(u)
                u = prev[u]
            path.reverse()
            if len(path) == len(sub) and len(path) - 1 == len(sedges) and len(path) == len(set(path)):
                paths.append(path)
        out.append(paths)
    return out


@pytest.mark.parametrize("name", [m["name"] for m in golden_cases()])
def test_bucketed_oracle_equals_predecessor_on_goldens(name):
    meta = [m for m in golden_cases() if m["name"] == name][0]
    cwd = os.getcwd()
    os.chdir(os.path.join(GOLDEN, "cases", name))
    try:
        state = go.load_and_build([r["tsv"] for r in meta["refs"]], [r["weight"] for r in meta["refs"]],
                                  meta["target"]["tsv"], meta["target"]["weight"])
    finally:
        os.chdir(cwd)
    for n in (1, 2, 3, 4):
        assert po.find_paths(state, n) == _find_paths_before(state, n), (name, n)


def test_bucketed_oracle_equals_predecessor_on_the_old_fuzz(tmp_path):
    """the first 20 trials of tests/test_gpu_paths.py::test_fuzz_paths_vs_oracle at its default seed (unique positions)"""
    from tests.test_gpu_paths import _write_random_assemblies
    rng = random.Random(4242)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        for t in range(20):
            names, weights = _write_random_assemblies(rng, t)
            state = go.load_and_build(names[:-1], weights[:-1], names[-1], weights[-1])
            for n in sorted({1, 2, 3, int(sum(weights)), int(sum(weights)) + 1}):
                assert po.find_paths(state, n) == _find_paths_before(state, n), (t, n)
    finally:
        os.chdir(cwd)
