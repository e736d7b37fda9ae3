"""GPU parity of mxg_find_paths on planned graphs (tests/_path_graphs.py): rings of every size class, equal positions,
vertex ids that do not follow the chain, branch nodes that need a filter round per threshold, the thresholds themselves,
degenerate graphs, the order of calls, and a seeded random corpus.  Every case is compared with oracle/paths_oracle.py
(whose graph comes from the plan's TSV files or arrays, never from the library) and checked for what holds without an
oracle: no vertex in two paths, every step of a path is an edge, sources in rising vertex index, the component count, and
the same arrays from three calls in a row."""
import os
import random

import numpy as np
import pytest

from oracle import paths_oracle as po
from tests import _path_graphs as pg

pytestmark = pytest.mark.gpu

BIG = 50000      # from here on the oracle state comes from the plan's arrays, not through TSV files (same state:
                 # tests/test_path_graphs_cpu.py::test_builder_routes_agree)


def _state(plan, tmp_path):
    return plan.state_from_arrays() if plan.n_vertices >= BIG else plan.state(str(tmp_path))


def _check(eng, graph, plan, state, n, repeats=3):
    """find_paths(n) against the oracle + the invariants; -> the paths as tuples of labels"""
    found = eng.find_paths(n)
    n_comp = eng.n_components
    for _ in range(repeats - 1):
        assert eng.find_paths(n) == found and eng.n_components == n_comp, ("calls differ", n)
    nv = len(plan.labels)
    lens = [len(p) for _c, p in found]
    flat = np.array([v for _c, p in found for v in p], dtype=np.int64)
    assert len(np.unique(flat)) == len(flat), ("a vertex is in two paths", n)
    assert all(ln >= 2 for ln in lens)
    if len(flat):
        inner = np.ones(len(flat), dtype=bool)
        inner[np.cumsum(lens) - 1] = False                   # the last vertex of a path has no step after it
        a, b = flat[:-1][inner[:-1]], flat[1:][inner[:-1]]
        eu, ev = graph["edge_u"].astype(np.int64), graph["edge_v"].astype(np.int64)
        keys = np.minimum(eu, ev) * nv + np.maximum(eu, ev)
        assert np.isin(np.minimum(a, b) * nv + np.maximum(a, b), keys).all(), ("a step is no edge", n)
    srcs = [p[0] for _c, p in found]
    assert srcs == sorted(srcs), ("sources not in rising vertex index", n)
    want = po.find_paths(state, n)
    assert n_comp == len(want), ("component count", n)
    names = state["vertices"]
    by_comp = {}
    for comp, verts in found:
        by_comp.setdefault(comp, []).append([names[v] for v in verts])
    assert po.canonical(by_comp.values()) == po.canonical(want), ("paths", n)
    return {tuple(plan.labels[v] for v in p) for _c, p in found}


def _run(plan, tmp_path, ns=(1,), repeats=3):
    """-> {n: set of paths as label tuples}"""
    from ntjoin_amd.engine import MxEngine
    state = _state(plan, tmp_path)
    out = {}
    with MxEngine(k=32, w=10) as eng:
        plan.load(eng)
        eng.build_graph()
        graph = eng.get_graph()
        # the plan's vertex order (place in the first assembly) is the library's: the oracle's tie rules speak of this index
        assert graph["vertex_hash"].tolist() == [plan.hash_of[lab] for lab in plan.labels]
        for n in ns:
            out[n] = _check(eng, graph, plan, state, n, repeats)
    return out


# ---- rings ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [(2, 1), (1, 2), (1, 1), (1, 2, 2)])
@pytest.mark.parametrize("L", [3, 4, 63, 64, 65, 256, 257, 70000])
def test_ring(L, weights, tmp_path):
    """opened by the positions of the FIRST top-weight assembly, oriented by those of the LAST: (1, 1) and (1, 2, 2) set them
    apart, and every assembly of pg.ring has another position order"""
    got = _run(pg.ring(L, weights), tmp_path)[1]
    assert got == {tuple(pg.ring_expected(L, weights))}


def test_many_rings_among_chains(tmp_path):
    plan = pg.rings_and_chains(2000, 5, 2000, 4)
    got = _run(plan, tmp_path)[1]
    assert got == ({tuple(("r", i, k) for k in range(5)) for i in range(2000)}
                   | {tuple(("c", i, k) for k in range(4)) for i in range(2000)})


def test_ring_with_no_path(tmp_path):
    assert _run(pg.ring_no_path(), tmp_path)[1] == set()


# ---- equal positions --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pg.tie_cases()))
def test_ties(name, tmp_path):
    """the rules of oracle/paths_oracle.py::find_paths, on the plan's state and on a state made of the library's own graph
    arrays (there "index" is the library's vertex index by construction); five calls give the same"""
    from ntjoin_amd.engine import MxEngine
    from tests.test_gpu_paths import _canonical_gpu, _state_from_graph
    plan, want = pg.tie_cases()[name]
    assert _run(plan, tmp_path, repeats=5)[1] == {tuple(p) for p in want}
    with MxEngine(k=32, w=10) as eng:
        plan.load(eng)
        eng.build_graph()
        state, _g = _state_from_graph(eng, plan.weights)
        for _ in range(5):
            assert _canonical_gpu(eng, 1) == po.canonical(po.find_paths(state, 1))


def test_many_rings_with_tied_neighbours(tmp_path):
    """3000 rings whose minimum vertex has two neighbours of equal position, each on a record of its own: which edge is
    cut must not depend on the order in which the neighbour slots were filled"""
    first, second = [], []
    for i in range(3000):
        lab = [(i, k) for k in range(6)]
        # even i: the minimum is vertex 0 of the ring (neighbours 1 and 5 tie), odd i: vertex 3 (neighbours 2 and 4 tie)
        first.append([pg.At(v, p) for v, p in zip(lab[:3], (5, 20, 30) if i % 2 == 0 else (10, 15, 20))])
        first.append([pg.At(v, p) for v, p in zip(lab[3:], (10, 15, 20) if i % 2 == 0 else (1, 20, 30))])
        second += [[lab[2], lab[3]], [lab[5], lab[0]], [lab[1]], [lab[4]]]
    plan = pg.Plan([(2, first), (1, second)], seed=7)
    got = _run(plan, tmp_path, repeats=5)[1]
    assert got == {tuple((i, k) for k in ((0, 5, 4, 3, 2, 1) if i % 2 == 0 else (3, 4, 5, 0, 1, 2))) for i in range(3000)}


# ---- vertex ids that do not follow the chain --------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["random", "reversed", "even_odd", "bit_reversed"])
@pytest.mark.parametrize("L", [1000, 70000])
def test_chain_ids_out_of_chain_order(L, order, tmp_path):
    """the first assembly holds every vertex as a record of its own, in an id order that scatters the chain: the component
    labelling must still finish"""
    assert _run(pg.chain(L, order), tmp_path)[1] == {tuple(range(L))}


# ---- branch nodes that need a round per threshold -----------------------------------------------------------------------
@pytest.mark.parametrize("weights", [(1, 2, 3), (0.5, 1, 1.5, 3)])
@pytest.mark.parametrize("branch_nodes", [10, 30000])
def test_ladder(branch_nodes, weights, tmp_path):
    """two branch nodes a rung, one of which stops being one a round before its neighbour"""
    rungs, top = branch_nodes // 2, len(weights) - 1
    got = _run(pg.ladder(rungs, weights), tmp_path)[1]
    assert got == {(("x", i, top), ("b", i), ("y", i)) for i in range(rungs)}


@pytest.mark.parametrize("weights", [(1, 2, 3), (0.5, 1, 1.5, 3)])
@pytest.mark.parametrize("branch_nodes", [10, 30000])
def test_comb(branch_nodes, weights, tmp_path):
    """one component of branch_nodes branch nodes; under (1, 2, 3) the backbone's ends stop being branch nodes a round early
    and keep their tooth of weight 2"""
    got = _run(pg.comb(branch_nodes, weights), tmp_path)[1]
    b = [("b", i) for i in range(branch_nodes)]
    assert got == {tuple([("t", 0, 1)] + b + [("t", branch_nodes - 1, 1)] if len(weights) == 3 else b)}


# ---- thresholds ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights,ns", [
    ((2, 1), (1, 2, 3, 4)),                 # n equal to an edge weight: `<` is strict; n = sum and sum + 1
    ((0.5, 1.5, 1), (1, 2, 3, 4)),          # 0.5 + 1.5 = 2.0 against n = 2
    ((1, 2, 3), (1, 2, 3, 6, 7)),           # n = floor(sum), floor(sum) + 1
    ((0.5, 1, 1.5, 3), (1, 2, 3, 6, 7)),
    ((2, 3), (1, 2, 3)),                    # n <= every weight: no global filter
    ((3, 3, 2), (1, 2, 3, 8, 9)),
    ((0.5, 0.5, 0.5), (0, 1, 2)),           # n = 0: nothing is below it
])
def test_thresholds(weights, ns, tmp_path):
    plans = [pg.mixed_chain(weights), pg.ladder(3, weights), pg.comb(5, weights)]
    if len(weights) == 3:
        plans.append(pg.star3(weights=weights))
    for plan in plans:
        _run(plan, tmp_path, ns)


def test_strict_threshold_literals(tmp_path):
    got = _run(pg.mixed_chain((0.5, 1.5, 1)), tmp_path, (2, 3))
    assert got[2] == {(0, 1, 2, 3), (4, 5, 6, 7), (8, 9, 10, 11)}       # the edge 4 - 5 weighs 0.5 + 1.5: not below 2
    assert got[3] == {(0, 1, 2), (6, 7), (10, 11)}                      # only the edges of all three assemblies
    # a branch node whose three edges are each shared by two of three assemblies of weight 0.5: no threshold up to the sum
    # of the weights is above an edge of weight 1, n = 0 included; the component stays branched and yields no path
    assert _run(pg.star3(), tmp_path, (0, 1, 2)) == {0: set(), 1: set(), 2: set()}


# ---- degenerate graphs ----------------------------------------------------------------------------------------------------
def test_no_shared_minimizer():
    from ntjoin_amd.engine import MxEngine
    with MxEngine(k=32, w=10) as eng:
        eng.add_minimizers("a", 2.0, [11, 12, 13], [0, 5, 9], [0, 0, 0], ["c"])
        eng.add_minimizers("b", 1.0, [21, 22], [0, 5], [0, 0], ["c"])
        eng.build_graph()
        for _ in range(3):
            assert eng.find_paths(1) == [] and eng.n_components == 0


def test_degenerate_graphs(tmp_path):
    singles = pg.Plan([(2, [[i] for i in range(300)]), (1, [[i] for i in range(299, -1, -1)])])     # vertices, no edge
    assert _run(singles, tmp_path, (1, 2))[1] == set()
    pairs = pg.Plan([(2, [[2 * i, 2 * i + 1] for i in range(700)]),
                     (1, [[2 * i + 1, 2 * i] for i in range(700)])])                                # components of two
    assert _run(pairs, tmp_path, (1, 3, 4))[1] == {(2 * i, 2 * i + 1) for i in range(700)}
    recs = [[("c", i, k) for k in range(3)] if i % 3 else [("s", i)] for i in range(900)]           # isolated among chains
    mixed = pg.Plan([(1, recs), (1, recs[::-1])])
    assert _run(mixed, tmp_path)[1] == {tuple(r) for r in recs if len(r) == 3}


# ---- order of calls -------------------------------------------------------------------------------------------------------
def test_n_3_then_1_then_3_on_one_handle(tmp_path):
    """every call is checked against the oracle, so the third must not see what the second left in the scratch"""
    for plan in (pg.ladder(5, (1, 2, 3)),
                 pg.perturbed_backbone(3000, random.Random(11), plant_rings=4, weights=[1, 2, 2, 0.5])):
        _run(plan, tmp_path, (3, 1, 3))


def test_large_graph_then_small_one(tmp_path):
    """fresh handles in one process: what the large graph left behind (scratch grows, never shrinks) is not the small one's"""
    assert _run(pg.chain(70000, "random"), tmp_path)[1] == {tuple(range(70000))}
    assert _run(pg.ring(3, (1, 1)), tmp_path)[1] == {(2, 1, 0)}
    assert _run(pg.tie_cases()["endpoints"][0], tmp_path)[1] == set()


# ---- the random corpus ------------------------------------------------------------------------------------------------------
CHUNKS = 4


@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_corpus(chunk, tmp_path):
    """tests/_path_graphs.py::corpus (what it reaches: tests/test_path_graphs_cpu.py::test_corpus_coverage) at
    n in {1, 2, 3, floor(sum of weights), floor(sum) + 1}; MXG_FUZZ_SEED / MXG_FUZZ_TRIALS as in test_fuzz_paths_vs_oracle"""
    seed = int(os.environ.get("MXG_FUZZ_SEED", str(pg.CORPUS_SEED)))
    trials = int(os.environ.get("MXG_FUZZ_TRIALS", str(pg.CORPUS_TRIALS)))
    n_paths = 0
    for t, plan in pg.corpus(seed, trials):
        if t % CHUNKS != chunk:
            continue
        got = _run(plan, tmp_path, pg.n_values(plan.weights), repeats=3)
        n_paths += sum(len(v) for v in got.values())
    assert n_paths > 0 or trials < CHUNKS
