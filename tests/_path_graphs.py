"""Planned minimizer graphs for the path stage (mxg_find_paths): shapes with a known answer, and a seeded random corpus.

A plan is a list of assemblies, each (weight, records); a record is an ordered list of vertex labels (consecutive labels of a
record become an edge), or of At(label, position) entries where a case needs its positions.  Every label occurs exactly once in
every assembly -- what the graph stage guarantees of its vertices -- so the graph's vertex index is the label's place in the
first assembly.  A plan gives, per assembly, the arrays MxEngine.add_minimizers takes, and the same data as TSV files for
oracle.graph_oracle.load_and_build: the expected paths never come from the library's own graph arrays.

Plain Python + numpy, no GPU import.
"""
import collections
import os
import random

import numpy as np

from oracle import graph_oracle as go


At = collections.namedtuple("At", "label pos")     # a record entry with an explicit position


class Plan:
    def __init__(self, assemblies, seed=0):
        self.weights = [float(w) for w, _recs in assemblies]
        self.records = []                       # per assembly: list of records, each a list of (label, position)
        for _w, recs in assemblies:
            out, at = [], 0
            for rec in recs:
                assert len(rec) > 0, "a record holds at least one vertex"
                row = []
                for item in rec:
                    at += 10                    # default positions: unique within the assembly, rising along the records
                    row.append(tuple(item) if isinstance(item, At) else (item, at))
                out.append(row)
            self.records.append(out)
        self.labels = [lab for rec in self.records[0] for lab, _p in rec]    # vertex index -> label
        self.check()
        rng = np.random.default_rng(seed)
        hs = np.unique(rng.integers(1, 2 ** 63, size=len(self.labels) + 1000, dtype=np.uint64))
        rng.shuffle(hs)
        self.hash_of = dict(zip(self.labels, hs[:len(self.labels)].tolist()))
        assert len(self.hash_of) == len(self.labels)
        self.tsv_names = [f"asm{a}.tsv" for a in range(len(self.weights))]
        self._arrays = {}

    def check(self):
        """every label exactly once in every assembly"""
        want = set(self.labels)
        assert len(want) == len(self.labels), "a label occurs twice in assembly 0"
        for a, recs in enumerate(self.records):
            seen = [lab for rec in recs for lab, _p in rec]
            assert len(seen) == len(want) and set(seen) == want, f"assembly {a} does not hold every label exactly once"

    # -- what the library takes ---------------------------------------------------------------------------------------
    def arrays(self, a):
        """hashes u64, pos u32, rec u32, ids: the arguments of MxEngine.add_minimizers for assembly a"""
        if a in self._arrays:
            return self._arrays[a]
        recs = self.records[a]
        hashes = np.array([self.hash_of[lab] for rec in recs for lab, _p in rec], dtype=np.uint64)
        pos = np.array([p for rec in recs for _lab, p in rec], dtype=np.uint32)
        rec = np.repeat(np.arange(len(recs), dtype=np.uint32), [len(r) for r in recs])
        self._arrays[a] = hashes, pos, rec, [f"c{r}" for r in range(len(recs))]
        return self._arrays[a]

    def load(self, eng):
        for a, w in enumerate(self.weights):
            eng.add_minimizers(self.tsv_names[a], w, *self.arrays(a))

    # -- what the oracle takes ----------------------------------------------------------------------------------------
    def write_tsvs(self, directory):
        for a, recs in enumerate(self.records):
            with open(os.path.join(directory, self.tsv_names[a]), "w", encoding="ascii") as fh:
                for r, rec in enumerate(recs):
                    fh.write(f"c{r}\t" + " ".join(f"{self.hash_of[lab]}:{p}:A" for lab, p in rec) + "\n")

    def _ordered(self, state):
        names = [str(self.hash_of[lab]) for lab in self.labels]
        assert set(names) == set(state["vertices"])
        state["vertices"] = names               # "index" of the oracle's tie rules = the library's vertex index
        return state

    def state(self, directory):
        """oracle state by the TSV route (graph_oracle.load_and_build), vertices in vertex-index order"""
        self.write_tsvs(directory)
        cwd = os.getcwd()
        os.chdir(directory)
        try:
            st = go.load_and_build(self.tsv_names[:-1], self.weights[:-1], self.tsv_names[-1], self.weights[-1])
        finally:
            os.chdir(cwd)
        return self._ordered(st)

    def state_from_arrays(self):
        """the same state from arrays(): no file in between"""
        info, mxs = {}, {}
        for a, nm in enumerate(self.tsv_names):
            hashes, pos, rec, ids = self.arrays(a)
            info[nm] = {str(h): (ids[r], p) for h, p, r in zip(hashes.tolist(), pos.tolist(), rec.tolist())}
            rows = [[] for _ in ids]
            for h, r in zip(hashes.tolist(), rec.tolist()):
                rows[r].append(str(h))
            mxs[nm] = rows
        weights = dict(zip(self.tsv_names, self.weights))
        filtered = go.filter_minimizers(mxs)
        vertices, edges = go.build_edges(filtered, weights)
        return self._ordered({"list_mx_info": info, "list_mxs": mxs, "weights": weights, "filtered": filtered,
                              "vertices": vertices, "edges": edges})

    def names(self, labels):
        """a path of labels as the oracle's vertex names"""
        return tuple(str(self.hash_of[lab]) for lab in labels)

    @property
    def n_vertices(self):
        return len(self.labels)


def _singles(labels):
    return [[lab] for lab in labels]


# ---- named shapes ---------------------------------------------------------------------------------------------------
def ring_rotation(L, a):
    """where assembly a's record of ring(L) starts"""
    return (a * max(1, L // 3)) % L


def ring(L, weights=(2, 1), seed=0):
    """one ring 0 - 1 - ... - L-1 - 0.  Assembly a holds it as one record that starts at label ring_rotation(L, a) and
    lacks the ring edge before it; two assemblies with different starts close the ring, and every assembly has another
    position order.  Expected (tests/test_path_graphs_cpu.py::RING_PATHS): opened before the start of the FIRST
    top-weight assembly's record, then oriented by the positions of the LAST one."""
    assert L >= 3 and len(weights) >= 2
    asms = []
    for a, w in enumerate(weights):
        r = ring_rotation(L, a)
        asms.append((w, [list(range(r, L)) + list(range(r))]))
    return Plan(asms, seed)


def rings_and_chains(n_rings, ring_len, n_chains, chain_len, seed=0):
    """n_rings rings and n_chains chains in one graph, vertex ids interleaved (ring, chain, ring, ...); weights (2, 1).
    Ring i = labels ("r", i, 0..), chain j = ("c", j, 0..); the second assembly closes every ring."""
    first, second = [], []
    for i in range(max(n_rings, n_chains)):
        if i < n_rings:
            lab = [("r", i, k) for k in range(ring_len)]
            first.append(lab)
            second.append([lab[-1], lab[0]])
            second.append(lab[1:-1])
        if i < n_chains:
            lab = [("c", i, k) for k in range(chain_len)]
            first.append(lab)
            second.append(lab[::-1])
    return Plan([(2, first), (1, second)], seed)


ID_ORDERS = ("identity", "random", "reversed", "even_odd", "bit_reversed")


def id_order(L, kind, seed=0):
    """vertex id -> place in the chain"""
    if kind == "identity":
        return list(range(L))
    if kind == "random":
        return np.random.default_rng(seed).permutation(L).tolist()
    if kind == "reversed":
        return list(range(L - 1, -1, -1))
    if kind == "even_odd":
        return list(range(0, L, 2)) + list(range(1, L, 2))
    if kind == "bit_reversed":
        bits = max(1, (L - 1).bit_length())
        return sorted(range(L), key=lambda x: int(format(x, f"0{bits}b")[::-1], 2))
    raise ValueError(kind)


def chain(L, id_order_kind="identity", weights=(1, 2, 1), seed=0):
    """one chain 0 - 1 - ... - L-1 carried by every assembly but the first, which holds every vertex as a record of its
    own in id order: the vertex ids do not follow the chain.  Expected: the one path 0 .. L-1."""
    order = id_order(L, id_order_kind, seed)
    return Plan([(weights[0], _singles(order))] + [(w, [list(range(L))]) for w in weights[1:]], seed)


def comb(backbone, weights=(1, 2, 3), seed=0):
    """one component: a backbone b0 - ... in the last (heaviest) assembly; in every lighter assembly a every backbone
    vertex has a tooth of its own (one edge of weight w_a).  Every backbone vertex is a branch node at first; the two ends of the backbone
    have one edge less and may stop being one a round before their neighbours do, and then keep a tooth."""
    A = len(weights)
    b = [("b", i) for i in range(backbone)]
    teeth = [[("t", i, a) for i in range(backbone)] for a in range(A - 1)]
    asms = []
    for a in range(A - 1):
        recs = [[b[i], teeth[a][i]] for i in range(backbone)]
        recs += _singles(t for c in range(A - 1) if c != a for t in teeth[c])
        asms.append((weights[a], recs))
    asms.append((weights[-1], [b] + _singles(t for c in range(A - 1) for t in teeth[c])))
    return Plan(asms, seed)


def ladder(rungs, weights=(1, 2, 3), seed=0):
    """`rungs` components of two branch nodes each.  In rung i the branch node ("b", i) lies between ("x", i, A-1) and
    ("y", i) in the last (heaviest) assembly and has a neighbour ("x", i, a) of its own in every lighter assembly a: it
    carries an edge of every single-assembly weight w1 < w2 < ..., and the loop needs a round per threshold until only
    the heaviest pair is left.  ("x", i, A-1) is a branch node too, by two edges of the lightest weight to ("p", i) and
    ("q", i): it stops being one a round (or more) before ("b", i) does.
    Expected at n = 1 with rising weights: the path x[A-1] - b - y of every rung."""
    A = len(weights)
    asms = []
    for a in range(A):
        recs = []
        for i in range(rungs):
            others = [("x", i, c) for c in range(A) if c != a] + [("y", i), ("p", i), ("q", i)]
            if a == A - 1:
                recs.append([("x", i, a), ("b", i), ("y", i)])
                others.remove(("y", i))
            else:
                recs.append([("b", i), ("x", i, a)])
            if a == 0:
                recs.append([("p", i), ("x", i, A - 1), ("q", i)])
                for lab in (("p", i), ("q", i), ("x", i, A - 1)):
                    others.remove(lab)
            recs += _singles(others)
        asms.append((weights[a], recs))
    return Plan(asms, seed)


def star3(seed=0, weights=(0.5, 0.5, 0.5)):
    """a vertex of degree 3 whose three edges are each shared by two of three assemblies: no threshold up to the sum of
    the weights is above an edge, so the component stays branched and yields no path"""
    return Plan([(weights[0], [["a", "v", "b"], ["c"]]), (weights[1], [["b", "v", "c"], ["a"]]),
                 (weights[2], [["c", "v", "a"], ["b"]])], seed)


def ring_expected(L, weights):
    """the path of ring(L, weights) as labels, from the rules alone: the ring is opened between the start r of the
    FIRST top-weight assembly's record (its smallest position) and r - 1 (the neighbour of larger position); of these two
    the one that comes first in the LAST top-weight assembly's record is the source"""
    top = max(weights)
    first = list(weights).index(top)
    last = len(weights) - 1 - list(weights)[::-1].index(top)
    r, r_last = ring_rotation(L, first), ring_rotation(L, last)
    if (r - r_last) % L < (r - 1 - r_last) % L:
        return [(r + i) % L for i in range(L)]
    return [(r - 1 - i) % L for i in range(L)]


def mixed_chain(weights, seed=0):
    """the chain 0 - ... - 11 without a branch: assembly a cuts it after every (a + 3)-th vertex, so its edges carry
    different sums of weights (the global filter's cases)"""
    L = 12
    return Plan([(w, [list(range(i, min(i + a + 3, L))) for i in range(0, L, a + 3)]) for a, w in enumerate(weights)], seed)


def _two_record_ring(pos0, pos1, seed):
    """ring 0 - 1 - 2 - 3 - 4 - 5 - 0: assembly 0 (weight 2) holds [0 1 2] and [3 4 5] with the given positions, assembly 1
    (weight 1) closes it with [2 3] and [5 0]"""
    return Plan([(2, [[At(i, p) for i, p in zip((0, 1, 2), pos0)], [At(i, p) for i, p in zip((3, 4, 5), pos1)]]),
                 (1, [[2, 3], [5, 0], [1], [4]])], seed)


# equal positions (they are per record, so two vertices on different records share one routinely).  TIE_CASES: name ->
# (plan, expected paths as labels); the rules are those of oracle/paths_oracle.py::find_paths
def tie_cases():
    return {
        # 0 and 3 share the ring's smallest position: 0, the lower index, is the minimum; its neighbours 1 (20) and 5 (30):
        # the edge 0 - 5 is cut
        "ring_min": (_two_record_ring((10, 20, 30), (10, 20, 30), 1), [[0, 1, 2, 3, 4, 5]]),
        # the neighbours 1 and 5 of the minimum 0 share a position: the edge to 1, the lower index, is cut
        "ring_neighbours_0": (_two_record_ring((5, 20, 30), (10, 15, 20), 2), [[0, 5, 4, 3, 2, 1]]),
        # the same for the minimum 3, whose lower neighbour 2 hangs on the edge that the OTHER assembly gave
        "ring_neighbours_3": (_two_record_ring((10, 15, 20), (1, 20, 30), 3), [[3, 4, 5, 0, 1, 2]]),
        # chain 0 - 1 - 2 - 3 whose endpoints share a position: 3, the later index, is source and target, no path
        "endpoints": (Plan([(2, [[At(0, 10), At(1, 20)], [At(2, 5), At(3, 10)]]), (1, [[1, 2], [0], [3]])], 4), []),
    }


def ring_no_path(seed=0):
    """ring 0 - 1 - 2 - 3 - 0 under weights (1, 1, 1): opened between 0 and 3 by assembly 0, whose two ends then have equal
    positions in assembly 2, the last top-weight one: no path"""
    return Plan([(1, [[0, 1, 2, 3]]), (1, [[3, 0], [1, 2]]),
                 (1, [[At(0, 10), At(1, 20)], [At(2, 5), At(3, 10)]])], seed)


def perturbed_backbone(V, rng, plant_rings=0, weights=None):
    """random graph of about V vertices: every assembly takes one shared backbone order and perturbs it -- short blocks
    moved or reversed, records cut at random, some records rotated -- which gives branch nodes that need several filter
    rounds, components that split on the way and many chains.  Positions restart in every record, so equal positions
    on different records are common.  Rings do not come up at random: a planted ring is a chain in one assembly whose
    last-to-first edge comes from a two-element record in another assembly.  rng is a random.Random."""
    if weights is None:
        weights = [rng.choice([1, 1, 2, 2, 0.5, 1.5, 3]) for _ in range(rng.choice([2, 3, 3, 4]))]
    A = len(weights)
    ring_sizes = [rng.choice([3, 4, 5, 8, 20, 70, 130]) for _ in range(plant_rings)]
    nb = max(2, V - sum(ring_sizes))
    mean_len = rng.choice([4, 12, 40, 200])
    per_asm = []
    for _a in range(A):
        order = list(range(nb))
        for _ in range(int(nb * rng.choice([0.005, 0.02, 0.05]))):
            i, n = rng.randrange(nb), rng.randint(1, 6)
            blk = order[i:i + n]
            if rng.random() < 0.5:
                order[i:i + n] = blk[::-1]
            else:
                del order[i:i + n]
                j = rng.randrange(len(order) + 1)
                order[j:j] = blk
        recs, i = [], 0
        while i < nb:
            n = 1 + int(rng.expovariate(1.0 / mean_len))
            rec = order[i:i + n]
            if len(rec) > 2 and rng.random() < 0.1:
                r = rng.randrange(1, len(rec))
                rec = rec[r:] + rec[:r]
            recs.append(rec)
            i += n
        per_asm.append(recs)
    for k, L in enumerate(ring_sizes):
        lab = [("ring", k, i) for i in range(L)]
        c = rng.randrange(A)
        d = rng.choice([a for a in range(A) if a != c])
        for a in range(A):
            if a == d:
                per_asm[a].append([lab[-1], lab[0]])
                if L > 2:
                    per_asm[a].append(lab[1:-1])
            elif a == c or rng.random() < 0.5:
                per_asm[a].append(list(lab))
            else:
                per_asm[a] += _singles(lab)
    asms = []
    for w, recs in zip(weights, per_asm):
        rng.shuffle(recs)
        out = []
        for rec in recs:                       # positions per record, from a few shared starts
            start, step = rng.choice([0, 0, 10, 50]), rng.choice([10, 10, 7])
            out.append([At(lab, start + step * i) for i, lab in enumerate(rec)])
        asms.append((w, out))
    return Plan(asms, seed=rng.getrandbits(32))


# ---- the seeded corpus (tests/test_path_graphs_cpu.py pins what it reaches; tests/test_gpu_path_shapes.py runs it) -----
CORPUS_SEED = 20261
CORPUS_TRIALS = 32
CORPUS_BIG = 20000        # every corpus has one graph of at least this many vertices (its first)


def corpus(seed=CORPUS_SEED, trials=CORPUS_TRIALS):
    """yields (trial, plan); no draw is skipped or refused.  Trial 0 is the large graph; every third trial has two
    assemblies that share the top weight."""
    rng = random.Random(seed)
    for t in range(trials):
        V = CORPUS_BIG + 500 if t == 0 else rng.choice([60, 300, 1200, 4000])
        weights = None
        if t % 3 == 0:
            weights = [rng.choice([0.5, 1, 1.5]) for _ in range(rng.choice([1, 2]))]
            top = rng.choice([2, 3])
            for _ in range(2):
                weights.insert(rng.randrange(len(weights) + 1), top)
        yield t, perturbed_backbone(V, rng, plant_rings=rng.choice([2, 4, 6]), weights=weights)


def n_values(weights):
    return sorted({1, 2, 3, int(sum(weights)), int(sum(weights)) + 1})
