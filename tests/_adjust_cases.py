"""Inputs of the path adjustment stage's tests: the hand-made cases that tests/golden/make_golden_adjust.py records, the goldens
as the restatement and the library take them, and the seeded generators (fuzz, ladder, strided, large) whose inputs are re-made
here while tests/golden/adjust/families holds what the reference answered on them.  Test infrastructure only.

A row is [contig, ori, start, end, contig_size, first_mx, terminal_mx, gap_size, raw_gap_size] (Ntjoin.format_paths)."""
import functools
import glob
import hashlib
import json
import os
import random

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adjust")


class _Rows:
    "rows with minimizer tags that differ from node to node"

    def __init__(self):
        self.tag = 1000

    def __call__(self, contig, ori, start, end, size=5000, gap=20, raw=None):
        self.tag += 2
        return [contig, ori, start, end, size, str(self.tag), str(self.tag + 1), gap, gap if raw is None else raw]


def hand_cases():
    """name -> dict(paths, no_cut, G).  No two overlapping segments of one contig begin at the same base: the order bedtools' sort
    gives such a pair is not pinned (tests/golden/adjust/README.md)."""
    cases = {}
    n = _Rows()
    cases["chains_plus"] = dict(no_cut=False, G=0, paths=[
        [n("A", "+", 0, 100), n("A", "+", 100, 250, gap=31), n("B", "+", 0, 500)],
        [n("C", "+", 0, 100), n("C", "+", 150, 300), n("C", "+", 300, 400, gap=7, raw=-5), n("D", "-", 10, 900)],
        [n("Z", "-", 0, 50), n("E", "+", 10, 20), n("E", "+", 30, 40), n("E", "+", 50, 60), n("E", "+", 70, 4000, gap=55)],
        [n("F", "+", 0, 10), n("F", "+", 5, 30), n("G", "+", 0, 30)],  # not ascending: stays two nodes (and the two overlap)
    ])
    cases["chains_minus"] = dict(no_cut=False, G=0, paths=[
        [n("A", "-", 500, 700), n("A", "-", 200, 400, gap=44), n("B", "+", 0, 500)],
        [n("B", "-", 600, 700), n("C", "-", 900, 1000), n("C", "-", 700, 900), n("C", "-", 100, 650, gap=3)],
        [n("E", "-", 700, 800), n("E", "-", 500, 600), n("E", "-", 300, 400), n("E", "-", 0, 200, gap=9), n("D", "+", 0, 90)],
        [n("F", "-", 0, 100), n("F", "-", 200, 300), n("F", "+", 400, 500), n("F", "-", 300, 350)],  # ascending '-', mixed: no merge
    ])
    cases["blocked"] = dict(no_cut=False, G=0, paths=[
        [n("A", "+", 0, 100), n("A", "+", 300, 400), n("B", "+", 0, 500)],
        [n("A", "+", 150, 250), n("C", "+", 0, 500)],
        [n("D", "-", 800, 900), n("D", "-", 100, 200), n("C", "+", 600, 700)],
        [n("B", "-", 600, 700), n("D", "+", 850, 1000)],  # reaches into [100, 900] of the '-' chain from the right
    ])
    cases["blocked_then_merged"] = dict(no_cut=False, G=0, paths=[
        [n("A", "+", 0, 100), n("A", "+", 500, 600, gap=12), n("B", "+", 0, 500)],
        [n("A", "+", 200, 300), n("A", "+", 400, 600, gap=77), n("C", "+", 0, 500)],
    ])
    cases["three_paths"] = dict(no_cut=False, G=0, paths=[
        [n("A", "+", 0, 100), n("A", "+", 120, 200), n("B", "+", 0, 500)],
        [n("C", "+", 0, 500), n("A", "-", 900, 1000), n("A", "-", 700, 800)],
        [n("A", "+", 300, 400), n("D", "+", 0, 100), n("A", "+", 450, 600)],
        [n("A", "+", 2000, 2100)],  # a path of one node: its segment is not tallied
    ])
    cases["overlaps"] = dict(no_cut=False, G=0, paths=[
        [n("A", "+", 1000, 3000), n("B", "+", 0, 500)],
        [n("A", "-", 1200, 1500), n("C", "+", 0, 500)],          # inside the longest: dropped, the path is left with one node
        [n("C", "-", 600, 900), n("A", "+", 500, 1100), n("D", "+", 0, 100)],   # reaches in from the left
        [n("D", "+", 200, 300), n("A", "-", 2900, 3500), n("E", "+", 0, 100)],  # ... from the right
        [n("A", "+", 3400, 3800), n("E", "+", 200, 300)],        # overlaps only what the first pass left of [2900, 3500]
        [n("E", "-", 400, 500), n("A", "+", 4000, 4100), n("A", "+", 4200, 4300)],  # untouched by all of it, and a merge
        [n("F", "+", 0, 1000), n("G", "+", 0, 10)],
        [n("F", "+", 900, 1200), n("G", "+", 20, 30)],
        [n("F", "+", 1100, 1250), n("G", "+", 40, 50)],
        [n("F", "+", 1240, 1300), n("G", "+", 60, 70), n("F", "+", 1245, 1290)],
    ])
    cases["question_nodes"] = dict(no_cut=False, G=0, paths=[
        [n("A", "+", 0, 100), n("A", "?", 100, 200), n("A", "+", 200, 300), n("B", "+", 0, 500)],
        [n("C", "+", 0, 100), n("C", "+", 100, 200, gap=5), n("D", "?", 0, 50, gap=9)],
        [n("E", "?", 0, 10), n("E", "?", 20, 30)],
    ])
    for name, G in (("no_cut", 0), ("no_cut_G100", 100)):
        cases[name] = dict(no_cut=True, G=G, paths=[
            [n("A", "+", 0, 400, size=1000), n("X", "+", 100, 300, size=300), n("A", "+", 600, 1000, size=1000, gap=13), n("B", "+", 0, 500)],
            [n("C", "+", 0, 200, size=900, gap=60), n("D", "+", 100, 400, size=800, gap=30), n("E", "-", 0, 50, size=50), n("F", "+", 0, 100)],
            [n("G", "+", 0, 700), n("D", "-", 500, 800, size=800, gap=45), n("H", "+", 0, 80, size=80)],   # D: equal lengths, the first is best
            [n("H", "-", 10, 40, size=80), n("C", "-", 300, 900, size=900), n("I", "+", 5, 95, size=100)],  # C: the longer one is best
            [n("J", "+", 0, 40, size=90), n("K", "+", 0, 10, size=10), n("J", "-", 50, 90, size=90), n("L", "+", 0, 5)],  # other orientation
            [n("M", "+", 0, 40, size=90), n("N", "+", 0, 10, size=10), n("M", "+", 50, 90, size=90), n("M", "+", 42, 48, size=90)],  # 3 regions
            [n("O", "+", 0, 40, size=90), n("P", "+", 0, 10, size=10), n("Q", "+", 2, 8, size=10), n("O", "+", 50, 90, size=90)],
            [n("P", "+", 2, 5, size=10), n("Q", "+", 0, 3, size=10), n("R", "+", 0, 10, size=10)],
        ])
    return cases


def load_goldens():
    out = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*.json"))):
        with open(path, encoding="ascii") as fh:
            out[os.path.basename(path)[:-5]] = json.load(fh)
    return out


# ---- rows <-> the library's arrays -------------------------------------------------------------------------------------------------
ORI = {"+": 0, "-": 1, "?": 2}
ORI_CHR = "+-?"


def to_arrays(paths, dtype, index=None):
    "rows -> (nodes of the given structured dtype, path_first, contig names by record)"
    names = sorted({row[0] for path in paths for row in path}) if index is None else None
    index = {c: r for r, c in enumerate(names)} if index is None else index
    flat = [row for path in paths for row in path]
    nodes = np.zeros(len(flat), dtype=dtype)
    nodes["record"] = [index[r[0]] for r in flat]
    nodes["ori"] = [ORI[r[1]] for r in flat]
    for j, name in ((2, "start"), (3, "end"), (4, "contig_size"), (7, "gap_size"), (8, "raw_gap_size")):
        nodes[name] = [r[j] for r in flat]
    nodes["first_mx"] = np.array([int(r[5]) for r in flat], dtype=np.uint64)
    nodes["terminal_mx"] = np.array([int(r[6]) for r in flat], dtype=np.uint64)
    first = np.cumsum([0] + [len(path) for path in paths]).astype(np.uint64)
    return nodes, first, names


def from_arrays(res, names):
    "the library's result -> (rows per path, source as (path, node) per path) given the input's path_first as res['in_first']"
    nd, first, src, in_first = res["nodes"], res["node_first"].tolist(), res["source"], res["in_first"]
    rows = [[names[r], ORI_CHR[o], s, e, cs, str(f), str(t), g, rg] for r, o, s, e, cs, f, t, g, rg in zip(
        nd["record"].tolist(), nd["ori"].tolist(), nd["start"].tolist(), nd["end"].tolist(), nd["contig_size"].tolist(),
        nd["first_mx"].tolist(), nd["terminal_mx"].tolist(), nd["gap_size"].tolist(), nd["raw_gap_size"].tolist())]
    p_of = np.searchsorted(in_first, src, side="right") - 1
    where = [(int(p), int(s - in_first[p])) for p, s in zip(p_of.tolist(), src.tolist())]
    return [rows[lo:hi] for lo, hi in zip(first, first[1:])], [where[lo:hi] for lo, hi in zip(first, first[1:])]


# ---- fuzz ---------------------------------------------------------------------------------------------------------------------------
FUZZ_SEEDS = list(range(200))


def fuzz_case(seed):
    """<= 40 paths over <= 12 contigs, <= 8 nodes per path.  Coordinates come from a coarse grid of the contig, so that nodes of
    different paths meet; runs of one contig in one orientation and in walking order are frequent, so that chains form."""
    rng = random.Random(seed)
    n_contigs = rng.randint(1, 12)
    sizes = [rng.choice([400, 1000, 3000]) for _ in range(n_contigs)]
    step = rng.choice([10, 25, 50])
    tag = [1]

    def row(c, ori, start, end):
        tag[0] += 2
        return [f"c{c}", ori, start, end, sizes[c], str(tag[0]), str(tag[0] + 1), rng.choice([0, 20, 20, 137]), rng.choice([-30, 0, 20, 137])]

    def span(c, lo=0):
        cells = sizes[c] // step
        a = rng.randint(min(lo, cells - 1), cells - 1)
        b = rng.randint(a + 1, min(cells, a + rng.choice([1, 2, 4, 10, cells])))
        return a * step, (b * step if rng.random() < 0.8 else b * step - rng.randint(1, step - 1))

    paths = []
    for _ in range(rng.randint(1, 40)):
        path, want = [], rng.randint(1, 8)
        while len(path) < want:
            c = rng.randrange(n_contigs)
            if rng.random() < 0.45 and want - len(path) >= 2:  # a run of one contig in walking order
                ori = rng.choice("++--?") if rng.random() < 0.1 else rng.choice("+-")
                k = rng.randint(2, min(4, want - len(path)))
                spans, at = [], 0
                for _k in range(k):
                    s, e = span(c, at)
                    spans.append((s, e))
                    at = -(-e // step) + rng.choice([0, 0, 1, 3])
                    if at >= sizes[c] // step:
                        break
                for s, e in (spans if ori != "-" else spans[::-1]):
                    path.append(row(c, ori if rng.random() < 0.93 else rng.choice("+-?"), s, e))
            elif rng.random() < 0.15 and len(path) >= 1 and want - len(path) >= 2:  # a contig between the two halves of another
                h = rng.randrange(n_contigs)
                cut = rng.randint(1, sizes[h] // step - 1) * step
                ori = rng.choice("+-")
                halves = [(0, cut), (cut + rng.choice([0, step]), sizes[h])] if ori == "+" else [(cut, sizes[h]), (0, cut)]
                path.append(row(h, ori, *halves[0]))
                path.append(row(c, rng.choice("+-"), *span(c)))
                if halves[1][0] < halves[1][1]:
                    path.append(row(h, ori, *halves[1]))
            else:
                path.append(row(c, rng.choice("++--?") if rng.random() < 0.2 else rng.choice("+-"), *span(c)))
        paths.append(path[:8])
    return dict(paths=paths, no_cut=seed % 2 == 1, G=rng.choice([0, 0, 100, 1000]))


def features(case, result, source):
    "what happened in a fuzz case: merges, blocked chains, overlaps resolved"
    from tests import _adjust_restatement as rs
    feats = set()
    n_in, n_out = sum(len(p) for p in case["paths"]), sum(len(p) for p in result)
    by_where = {w: row for path, ws in zip(result, source) for row, w in zip(path, ws)}
    for p, path in enumerate(case["paths"]):
        for i, row in enumerate(path):
            out = by_where.get((p, i))
            if out is not None and out[3] - out[2] > row[3] - row[2] and not case["no_cut"]:
                feats.add("merge")
            if out is not None and (out[2] > row[2] or out[3] < row[3]):
                feats.add("overlap_cut")
    if n_out < n_in:
        feats.add("dropped")
    for path, ws in zip(result, source):  # two neighbours that would have merged, had nothing been in the way
        for a, b in zip(path, path[1:]):
            if a[0] == b[0] and a[1] == b[1] and ((a[1] == "+" and a[3] <= b[2]) or (a[1] == "-" and a[2] >= b[3])):
                feats.add("blocked")
    sets = {}
    for path in case["paths"]:
        if len(path) >= 2:
            for row in path:
                sets.setdefault(row[0], set()).add((row[2], row[3]))
    if any(c > 1 for segs in sets.values() for _s, c in rs.intersection_counts(segs)):
        feats.add("overlap")
    return feats


def duplicate_case():
    "two nodes with the same contig, start and end, one of which merges: the second merge finds the segment gone (path 1, node 1)"
    n = _Rows()
    return dict(no_cut=False, G=0, paths=[
        [n("A", "+", 0, 100), n("A", "+", 100, 200), n("B", "+", 0, 500)],
        [n("A", "+", 0, 100), n("A", "+", 300, 400), n("C", "+", 0, 500)],
    ])


def strided_case(no_cut=False):
    "a contig with 200 segments in 200 paths, a chain of 70 nodes, and a contig whose set holds more than 64 segments while chains merge"
    rng = random.Random(77)
    n = _Rows()
    paths, seen = [], set()
    while len(paths) < 200:
        s = rng.randrange(0, 99000, 10)
        e = s + rng.choice([10, 50, 300, 2000])
        if (s, e) in seen or any(s == s2 for s2, _ in seen):
            continue
        seen.add((s, e))
        paths.append([n("BIG", rng.choice("+-"), s, e, size=101000), n(f"o{len(paths)}", "+", 0, 100, size=100)])
    paths.append([n("CH", "+", 100 * i, 100 * i + 60 + (i % 3) * 20, size=7000, gap=i) for i in range(70)] + [n("Z", "+", 0, 10)])
    for i in range(40):  # MIX: 80 singles, then chains between them
        paths.append([n("MIX", "-", 100000 - 1000 * i - 300, 100000 - 1000 * i - 200, size=100000),
                      n("MIX", "-", 100000 - 1000 * i - 600, 100000 - 1000 * i - 500, size=100000), n(f"m{i}", "+", 0, 50, size=100)])
        paths.append([n(f"m{i}", "-", 60, 90, size=100), n("MIX", "+", 1000 * i + 450, 1000 * i + 480 + (40 if i % 5 == 0 else 0), size=100000)])
    return dict(no_cut=no_cut, G=50 if no_cut else 0, paths=paths)


def check_case(case):
    """What every input must keep, since ntJoin holds one length per contig (from the FASTA) and neither the library nor the
    restatement checks it: one contig_size per contig, 0 <= start < end <= contig_size, an orientation of + - ?"""
    sizes = {}
    for p, path in enumerate(case["paths"]):
        for i, row in enumerate(path):
            contig, ori, start, end, size = row[:5]
            assert sizes.setdefault(contig, size) == size, (p, i, contig, sizes[contig], size)
            assert 0 <= start < end <= size, (p, i, row)
            assert ori in ("+", "-", "?"), (p, i, row)
    return case


LADDER_L = [2, 3, 63, 64, 65, 127, 128, 129, 200, 257]  # around the wave (64, 128) and the block (256)
LADDER_PATHS = [(255, False), (256, True), (257, False)]  # (paths, no_cut): around the block of the per-path kernels, which run P + 1 threads


def ladder_case(L, no_cut=False, n_paths=None):
    """Contigs X and Y in exactly L nodes each.  X: chains of 1 to 3 nodes in walking order, 0, 5, 10 or 40 bases apart, in both
    orientations, and single nodes hooked into the segment before them (begun 25 to 29 bases before its end, or inside it); all
    starts differ, so the order of equal starts stays out.  Y: triples Y+ (a, a+50), Y+ (a+100, a+150) in one path and
    Y- (a+60, a+90) in another, which blocks the chain, then singles of 70 bases, two and two sharing 25 of them; the path that
    comes last holds such a single, so that Y's list ends in a segment that counts.  Every path ends in a contig of its own, some
    begin with one.  n_paths: two-node paths of contigs of their own are added up to that many paths."""
    rng = random.Random(1000 + 2 * L + int(no_cut) + (0 if n_paths is None else 7 * n_paths))
    size, tag, own = 1000 * L + 1000, [1], [0]

    def row(contig, ori, start, end, csize):
        tag[0] += 2
        return [contig, ori, start, end, csize, str(tag[0]), str(tag[0] + 1), rng.choice([0, 20, 137]), rng.choice([-30, 0, 20, 137])]

    def close(nodes):
        own[0] += 1
        lead = [row(f"lead{own[0]}", rng.choice("+-"), 10, 90, 100)] if rng.random() < 0.3 else []
        return lead + nodes + [row(f"own{own[0]}", rng.choice("+-"), 0, 100, 100)]

    paths, left, at, last, can_hook = [], L, 100, None, False
    while left:  # X
        kind = rng.random()
        if can_hook and kind < 0.3:  # reaches 25 to 29 bases back into the segment before it
            start = last[1] - rng.randint(25, 29)
            spans = [(start, start + rng.choice([50, 100, 200]))]
            can_hook = False
        elif can_hook and kind < 0.4:  # inside the segment before it
            spans, can_hook = [(last[0] + 10, last[1] - 10)], False
        else:
            spans = []
            for _ in range(min(left, rng.choice([1, 1, 1, 2, 3]))):
                spans.append((at, at + rng.choice([50, 100, 200])))
                at = spans[-1][1] + rng.choice([0, 5, 10, 40])
            can_hook = True
        last = spans[-1] if can_hook else last
        at = max(at, spans[-1][1]) + rng.choice([10, 60])
        ori = rng.choice("+-")
        paths.append(close([row("X", ori, s, e, size) for s, e in (spans if ori == "+" else spans[::-1])]))
        left -= len(spans)
    a = 100
    for _ in range(L // 5):  # Y: the '-' node of another path lies between the two '+' nodes
        paths.append(close([row("Y", "+", a, a + 50, size), row("Y", "+", a + 100, a + 150, size)]))
        paths.append(close([row("Y", "-", a + 60, a + 90, size)]))
        a += 200
    tail = None
    for j in range(L - 3 * (L // 5)):  # ... then singles, two and two sharing 25 bases
        paths.append(close([row("Y", rng.choice("+-"), a + 45 * (j % 2), a + 45 * (j % 2) + 70, size)]))
        tail = paths[-1] if j % 2 else tail
        a += 200 * (j % 2)
    while n_paths is not None and len(paths) < n_paths:
        k = len(paths)
        paths.append([row(f"pad{k}a", rng.choice("+-"), 10, 90, 100), row(f"pad{k}b", rng.choice("+-"), 0, 100, 100)])
    assert n_paths is None or len(paths) == n_paths
    rng.shuffle(paths)
    paths.remove(tail)  # the last entry of Y's list and of its set of segments is one that intersects another
    paths.append(tail)
    return dict(paths=paths, no_cut=no_cut, G=rng.choice([0, 100]))


@functools.lru_cache(maxsize=None)
def large_case(n_nodes=100000, n_contigs=30000, seed=5):
    "10^5 nodes over 3 * 10^4 contigs of 11000 bases (a run ends before 10800) in paths of up to 8 nodes; no (contig, start, end) twice.  Cached: read it, do not change it"
    rng = random.Random(seed)
    paths, seen, total, tag = [], set(), 0, 1
    while total < n_nodes:
        path = []
        want = min(rng.randint(1, 8), n_nodes - total)
        while len(path) < want:
            c = rng.randrange(n_contigs)
            run = rng.randint(1, min(3, want - len(path))) if rng.random() < 0.5 else 1
            ori = rng.choice("+-")
            at = rng.randrange(0, 9000)
            spans = []
            for _ in range(run):
                e = at + rng.choice([50, 100, 100, 400])
                spans.append((at, e))
                at = e + rng.choice([0, 100, 300])
            for s, e in (spans if ori == "+" else spans[::-1]):
                if (c, s, e) in seen:
                    continue
                seen.add((c, s, e))
                tag += 2
                path.append([f"c{c}", ori, s, e, 11000, str(tag), str(tag + 1), rng.choice([0, 20, 137]), rng.choice([-30, 20, 137])])
        paths.append(path[:want])
        total += len(paths[-1])
    from tests import _adjust_restatement as rs
    while True:  # (a merged segment may equal one that is there already: such a path is emptied, the node count stays close)
        try:
            return dict(paths=paths, no_cut=False, G=0, expected=rs.adjust(paths, False, 0))
        except KeyError as err:
            paths[err.args[0][0]] = paths[err.args[0][0]][:1]


# ---- families: seeded inputs re-made here, the reference's answers under tests/golden/adjust/families ------------------------------
GENERATORS = {"fuzz_case": fuzz_case, "ladder_case": ladder_case, "strided_case": strided_case, "large_case": large_case}
LARGE_HEAD = 50  # output paths of the large case that its golden holds verbatim


def family_specs():
    "family -> [(case name, generator, arguments)]: what make_golden_adjust.py records and the tests read back"
    ladder = [(f"L{L}" + ("_no_cut" if no_cut else ""), "ladder_case", dict(L=L, no_cut=no_cut)) for L in LADDER_L for no_cut in (False, True)]
    ladder += [(f"paths{P}", "ladder_case", dict(L=3, no_cut=no_cut, n_paths=P)) for P, no_cut in LADDER_PATHS]
    return {
        "fuzz": [(f"seed{seed:03d}", "fuzz_case", dict(seed=seed)) for seed in FUZZ_SEEDS],
        "ladder": ladder,
        "strided": [("strided" + ("_no_cut" if no_cut else ""), "strided_case", dict(no_cut=no_cut)) for no_cut in (False, True)],
        "large": [("large", "large_case", {})],
    }


def case_digest(case):
    return hashlib.sha256(json.dumps([case["paths"], case["no_cut"], case["G"]], separators=(",", ":")).encode("ascii")).hexdigest()


def json_digest(value):
    return hashlib.sha256(json.dumps(value, separators=(",", ":")).encode("ascii")).hexdigest()


def summarise_large(result, source):
    "what the large case's golden holds in place of its rows"
    lists = lambda v: json.loads(json.dumps(v))
    assert all(len(path) <= 9 for path in result)  # counts: one digit per output path
    return dict(result_sha256=json_digest(lists(result)), source_sha256=json_digest(lists(source)), counts="".join(str(len(path)) for path in result),
                result_head=lists(result[:LARGE_HEAD]), source_head=lists(source[:LARGE_HEAD]))


def pack_result(case, result, source):
    """The reference's answer next to the input it was given, without loss: per output path, per node either i, the input node of
    the same path that it is, unchanged, or [i, column, value, ...] with the columns of the row that differ.  The stage never
    moves a node to another path; asserted here, when the golden is recorded"""
    packed = []
    for p, (path, where) in enumerate(zip(result, source)):
        nodes = []
        for row, (q, i) in zip(path, where):
            was = case["paths"][p][i]
            assert q == p and len(row) == len(was), (p, i, row, was)
            nodes.append(i if row == was else [i] + [x for j in range(len(row)) if row[j] != was[j] for x in (j, row[j])])
        packed.append(nodes)
    assert unpack_result(case, packed) == (result, source)
    return packed


def unpack_result(case, packed):
    "-> (result, source) as the reference returned them"
    result, source = [], []
    for p, nodes in enumerate(packed):
        rows = []
        for node in nodes:
            row = list(case["paths"][p][node if isinstance(node, int) else node[0]])
            for j, value in ([] if isinstance(node, int) else zip(node[1::2], node[2::2])):
                row[j] = value
            rows.append(row)
        result.append(rows)
        source.append([[p, node if isinstance(node, int) else node[0]] for node in nodes])
    return result, source


@functools.lru_cache(maxsize=None)
def load_family(family):
    """-> {case name: golden document with "case" (the input, re-made and checked against the recorded digest) and, from its
    packed "nodes", "result" and "source"}.  Cached: read it, do not change it"""
    with open(os.path.join(GOLDEN, "families", family + ".json"), encoding="ascii") as fh:
        doc = json.load(fh)
    out = {}
    for entry in doc["cases"]:
        meta = entry["meta"]
        case = GENERATORS[meta["generator"]](**meta["args"])
        assert case_digest(case) == meta["sha256"], f"{family}/{meta['name']}: the generator no longer gives the input the golden was recorded on"
        entry = dict(entry, case=case)
        if "nodes" in entry:
            entry["result"], entry["source"] = unpack_result(case, entry.pop("nodes"))
        out[meta["name"]] = entry
    return out
