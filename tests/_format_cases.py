"""Inputs of the path stage's pin to ntJoin's own find_paths and format_path: the seeded and hand-made generators that
tests/golden/make_golden_format.py records and that tests/test_format_pin_cpu.py and tests/test_gpu_format_pin.py re-make, and the
reader of tests/golden/format/families.  Plain Python: no GPU, no reference import.  Test infrastructure only.

An assembly is a list of (record id, [(hash, pos), ...]), as _add() of tests/test_gpu_format_paths.py takes it.  A case is a dict
with asms (references first, target last), weights, lengths (target contig -> length), k, n, g, G and m; hand-made cases also
carry doc (the expected arithmetic), tags (the kinds of junction they hold) and expect (the (gap, raw) of every junction, by path).
A row is [contig, ori, start, end, contig_size, first_mx, terminal_mx, gap_size, raw_gap_size] (format_path)."""
import functools
import hashlib
import json
import os
import random

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "format")
K = 32


def _random_assemblies(rng):
    """two references and a target over one universe of minimizers: collinear stretches with drop-outs, reversed stretches,
    shuffled stretches and single minimizers as contigs; unique positions per assembly (the reference leaves ties to set order)"""
    universe = [rng.getrandbits(62) + 1 for _ in range(rng.choice([40, 120, 400]))]
    asms, lengths = [], {}
    for a in range(3):
        recs, at = [], 0
        keep = rng.choice([0.7, 0.85, 1.0]) if a < 2 else 1.0
        while at < len(universe):
            n = rng.choice([1, 1, 2, 3, 5, 8, 20, 70]) if a == 2 else rng.choice([2, 3, 5, 20, 70])
            picks = [h for h in universe[at:at + n] if rng.random() < keep]
            at += n
            mode = rng.random()
            if a == 2 and mode < 0.25:
                picks.reverse()
            elif a == 2 and mode < 0.5 and len(picks) > 2:
                i, j = rng.randrange(len(picks)), rng.randrange(len(picks))
                picks[i], picks[j] = picks[j], picks[i]
            elif a == 2 and mode < 0.6:
                rng.shuffle(picks)
            if picks:
                recs.append(picks)
        total = sum(len(p) for p in recs)
        pool = sorted(rng.sample(range(10 ** 6), total))
        rng.shuffle(recs)
        out, at = [], 0
        for r, picks in enumerate(recs):
            pos = pool[at:at + len(picks)]
            at += len(picks)
            if a == 2:  # the target's positions are contig-local: overhangs of tens of bases, as on real contigs
                shift = pos[0] - rng.randrange(60)
                pos = [p - shift for p in pos]
                lengths[f"ctg{r}"] = pos[-1] + K + rng.randrange(60)
            out.append((f"ctg{r}", list(zip(picks, pos))))
        asms.append(out)
    return asms, lengths


# ---- fuzz ---------------------------------------------------------------------------------------------------------------------------
FUZZ_CASES = 60
FUZZ_WEIGHTS = [(1.0, 1.0, 1.0), (2.0, 1.0, 1.0), (1.0, 2.0, 1.0), (2.0, 2.0, 1.0)]


@functools.lru_cache(maxsize=None)
def _fuzz_draws():
    "the first FUZZ_CASES draws of the sequence test_fuzz_against_host_route walks (its 12 trials are the first 12)"
    rng = random.Random(20)
    draws = []
    for _ in range(FUZZ_CASES):
        asms, lengths = _random_assemblies(rng)
        draws.append((asms, lengths, rng.choice(FUZZ_WEIGHTS)))
    return draws


def fuzz_case(i):
    asms, lengths, weights = _fuzz_draws()[i]
    return dict(asms=asms, weights=list(weights), lengths=lengths, k=K, n=1 if i % 4 else 2, g=(1, 20)[i // 3 % 2], G=(0, 40)[i // 6 % 2],
                m=(50, 75, 90)[i % 3])


# ---- chains: the hand-made cases ----------------------------------------------------------------------------------------------------
def _h(i):
    return 1_000_003 * (i + 1)


def chain_case(chains, refs=({},), loose=(), lengths=None, weights=None, n=2, g=20, G=0, m=90, **extra):
    """chains: lists of (target contig, position) in walking order; minimizer number i of chain c is its own hash.  Every
    reference (weight 2) holds chain c as record chr<c> with positions step * (i + 1), cut into records in front of the items
    in cuts[c]; with n = 2 the target's own edges (weight 1) fall to the global filter, so the paths are the chains, walked
    upwards.  loose: (contig, position) of target minimizers that every reference holds alone in a record: graph vertices on
    no path.  A target contig is every item of that name, wherever it lies."""
    items = [(c, i, ctg, pos) for c, chain in enumerate(chains) for i, (ctg, pos) in enumerate(chain)]
    hashes = {(c, i): _h(j) for j, (c, i, _ctg, _pos) in enumerate(items)}
    loose_h = [_h(len(items) + j) for j in range(len(loose))]
    asms = []
    for ref in refs:
        step, cuts = ref.get("step", 1000), ref.get("cuts", {})
        recs = []
        for c, chain in enumerate(chains):
            for i in range(len(chain)):
                if i == 0 or i in cuts.get(c, ()):
                    recs.append((f"chr{c}" if i == 0 else f"chr{c}.{i}", []))
                recs[-1][1].append((hashes[(c, i)], step * (i + 1)))
        recs += [(f"lone{j}", [(h, 1000)]) for j, h in enumerate(loose_h)]
        asms.append(recs)
    target = {}
    for c, i, ctg, pos in items:
        target.setdefault(ctg, []).append((hashes[(c, i)], pos))
    for (ctg, pos), h in zip(loose, loose_h):
        target.setdefault(ctg, []).append((h, pos))
    for ctg, mxs in target.items():
        assert len({p for _h, p in mxs}) == len(mxs), f"{ctg}: two minimizers at one position"
    asms.append(list(target.items()))
    full = {ctg: 1000 for ctg in target}
    full.update(lengths or {})
    assert set(full) == set(target)
    return dict(asms=asms, weights=list(weights or [2.0] * len(refs) + [1.0]), lengths=full, k=K, n=n, g=g, G=G, m=m, **extra)


def _up(ctg, n=5, step=100, at=100):
    return [(ctg, at + step * i) for i in range(n)]


def _down(ctg, n=5, step=100, at=100):
    return _up(ctg, n, step, at)[::-1]


def _mixed(ctg, n, seed=0, step=10, at=10):
    "n >= 3 positions that the m rule leaves without an orientation at every m >= 75; one minimizer has none either"
    return [(ctg, at + step * p) for p in _shuffle_mixed(random.Random(1000 * n + seed), list(range(n)))]


# -- m_rule
def _pairs_run(inc, d):
    "d + 1 distinct positions with exactly inc increasing consecutive pairs, the increasing ones spread evenly among the others"
    pos, hi, lo, acc = [0], 0, 0, 0
    for _ in range(d):
        acc += inc
        if acc >= d:
            acc -= d
            hi += 10
            pos.append(hi)
        else:
            lo -= 10
            pos.append(lo)
    pos = [p - lo + 10 for p in pos]
    assert len(set(pos)) == d + 1 and sum(a < b for a, b in zip(pos, pos[1:])) == inc and sum(a > b for a, b in zip(pos, pos[1:])) == d - inc
    return pos


M_RULE_FLOAT = [(29, 50, 58, "?"), (29, 100, 29, "-"), (57, 100, 57, "?"), (58, 100, 58, "?"), (87, 150, 58, "?"), (58, 200, 29, "-"),
                (114, 200, 57, "?"), (116, 200, 58, "?")]   # (inc, d, m, what inc / float(d) * 100 >= m decides): exact arithmetic says '+'


def m_rule_case(inc, d, m, mirror=False):
    """one path A - U - C as _abc() of tests/test_gpu_format_paths.py builds it: U holds d + 1 minimizers with exactly inc
    increasing pairs (mirror: U walked backwards, so d - inc of them)"""
    pos = _pairs_run(inc, d)
    if mirror:
        pos = pos[::-1]
        assert sum(a < b for a, b in zip(pos, pos[1:])) == d - inc
    chain = _up("A") + [("U", p) for p in pos] + _up("C")
    return chain_case([chain], lengths={"U": max(pos) + 100}, m=m, u_pairs=[d + 1, d - inc if mirror else inc, inc if mirror else d - inc])


def _m_rule_specs():
    specs = []
    for inc, d, m, _float in M_RULE_FLOAT:
        specs.append((f"float_{inc}_{d}_m{m}", dict(inc=inc, d=d, m=m)))
        specs.append((f"float_{inc}_{d}_m{m}_mirror", dict(inc=inc, d=d, m=m, mirror=True)))
    for inc, d, m in ((9, 10, 90), (1, 10, 90), (3, 4, 75), (1, 4, 75), (8, 10, 90), (2, 10, 90), (2, 4, 75)):
        specs.append((f"boundary_{inc}_{d}_m{m}", dict(inc=inc, d=d, m=m)))
    for d in (10, 64):   # m = 100: one pair out of order in a run of 11 and of 65
        specs.append((f"m100_run{d + 1}", dict(inc=d - 1, d=d, m=100)))
        specs.append((f"m100_run{d + 1}_mirror", dict(inc=d - 1, d=d, m=100, mirror=True)))
    for d in (2, 10, 64):   # m = 50, half the pairs: both tests hold, '+' is asked first
        specs.append((f"m50_half_{d}", dict(inc=d // 2, d=d, m=50)))
    specs.append(("two_minimizers_up", dict(inc=1, d=1, m=90)))
    specs.append(("two_minimizers_down", dict(inc=0, d=1, m=90)))
    return [(name, "m_rule_case", args) for name, args in specs]


# -- gaps
GAP_TAGS = ("ori++", "ori+-", "ori-+", "ori--", "u_whole", "u_cut", "v_whole", "v_cut", "cut_same_path", "cut_other_path", "cut_no_path",
            "support1", "support2", "support3", "trunc.5", "trunc.33", "trunc.67", "raw_negative", "raw_g-1", "raw_g", "raw_g+1", "raw_G-1",
            "raw_G", "raw_G+1", "stretch1", "stretch63", "stretch64", "stretch65", "stretch300", "empty_support", "last_run_unoriented",
            "only_unoriented", "a_negative", "b_negative")


def _gap_table():
    """name -> (doc, tags, expect, case).  The standard junction: u = A, v = C, five minimizers each at 100 .. 500, both 1000 long,
    one reference with 1000 between neighbours: mean = 1000 - 32 = 968.  Whole: a = 1000 - 500 - 32 = 468 ('+') or 100 - 0 ('-');
    b = 100 - 0 ('+') or 1000 - 500 - 32 = 468 ('-').  Cut on both sides (start 100, end 532): a = b = 0."""
    t = {}

    def add(name, doc, tags, expect, case):
        assert name not in t and set(tags) <= set(GAP_TAGS), name
        t[name] = (doc, tuple(tags), expect, case)

    run = {"+": _up, "-": _down}
    a_whole, b_whole = {"+": 468, "-": 100}, {"+": 100, "-": 468}
    for uo in "+-":
        for vo in "+-":
            raw = 968 - a_whole[uo] - b_whole[vo]
            add(f"whole_{uo}{vo}", f"A({uo}) C({vo}) whole: raw = 968 - {a_whole[uo]} - {b_whole[vo]} = {raw}", [f"ori{uo}{vo}", "u_whole", "v_whole", "support1", "stretch1"],
                [[(raw, raw)]], chain_case([run[uo]("A") + run[vo]("C")]))
            add(f"cut_{uo}{vo}", f"A({uo}) C({vo}), each with a vertex on no path at 50 and at 900: 100-532, a = b = 0, raw = 968",
                [f"ori{uo}{vo}", "u_cut", "v_cut", "cut_no_path"], [[(968, 968)]],
                chain_case([run[uo]("A") + run[vo]("C")], loose=[("A", 50), ("A", 900), ("C", 50), ("C", 900)]))
    # cut on one side only, by a vertex in the same path, in another path, on no path
    add("u_cut_same_path", "A(+) C(+) A(+): A's second run 1100 .. 1500 cuts the first at 532, a = 0; raw = 968 - 0 - 100 = 868; C -> A: a = 468, b = 1100 - 1100 = 0, raw = 500",
        ["ori++", "u_cut", "v_whole", "cut_same_path", "v_cut"], [[(868, 868), (500, 500)]],
        chain_case([_up("A") + _up("C") + _up("A", at=1100)], lengths={"A": 2000}))
    add("v_cut_same_path", "C(-) A(-) C(-): C's runs 1500 .. 1100 and 500 .. 100; C1 -> A: a = 1100 - 1100 = 0, b = 468, raw = 500; A -> C2: a = 100, b = 532 - 500 - 32 = 0, raw = 868",
        ["ori--", "u_cut", "v_cut", "u_whole", "cut_same_path"], [[(500, 500), (868, 868)]],
        chain_case([_down("C", at=1100) + _down("A") + _down("C")], lengths={"C": 2000}))
    add("u_cut_other_path", "path 0: A(+) C(+), path 1: D(+) A(+) with A at 1100 .. 1500: A ends at 532 in path 0 (a = 0, raw = 868) and starts at 1100 in path 1 (a = 468, b = 0, raw = 500)",
        ["ori++", "u_cut", "v_cut", "cut_other_path"], [[(868, 868)], [(500, 500)]],
        chain_case([_up("A") + _up("C"), _up("D") + _up("A", at=1100)], lengths={"A": 2000}))
    add("v_cut_other_path", "path 0: A(-) C(-), path 1: C(+) D(+) with C at 1100 .. 1500 (C is 2000 long): C is 0-532 in path 0, b = 532 - 500 - 32 = 0, raw = 968 - 100 - 0 = 868; path 1: C 1100-2000, a = 2000 - 1500 - 32 = 468, raw = 400",
        ["ori--", "v_cut", "u_whole", "cut_other_path"], [[(868, 868)], [(400, 400)]],
        chain_case([_down("A") + _down("C"), _up("C", at=1100) + _up("D")], lengths={"C": 2000}))
    add("u_cut_no_path", "A(+) C(+), A holds a vertex on no path at 900: A is 0-532, a = 0, raw = 968 - 0 - 100 = 868", ["ori++", "u_cut", "v_whole", "cut_no_path"],
        [[(868, 868)]], chain_case([_up("A") + _up("C")], loose=[("A", 900)]))
    add("v_cut_no_path", "A(+) C(+), C holds a vertex on no path at 50: C is 100-1000, b = 0, raw = 968 - 468 - 0 = 500", ["ori++", "u_whole", "v_cut", "cut_no_path"],
        [[(500, 500)]], chain_case([_up("A") + _up("C")], loose=[("C", 50)]))
    add("u_start_cut_only", "A(-) C(+), A holds a vertex on no path at 900: A is 0-532 walked downwards, a = 100 - 0, raw = 968 - 100 - 100 = 768", ["ori-+", "u_cut", "cut_no_path"],
        [[(768, 768)]], chain_case([_down("A") + _up("C")], loose=[("A", 900)]))
    add("u_cut_m_rule", "A = 100 200 300 500 400 (3 of 4 pairs, '+' at m = 75) with a vertex on no path at 900: end = 532, the last minimizer is at 400: a = 532 - 400 - 32 = 100; raw = 968 - 100 - 100 = 768",
        ["ori++", "u_cut", "cut_no_path"], [[(768, 768)]],
        chain_case([[("A", p) for p in (100, 200, 300, 500, 400)] + _up("C")], loose=[("A", 900)], m=75))
    add("v_cut_m_rule", "C = 200 100 300 400 500 (3 of 4 pairs, '+' at m = 75) with a vertex on no path at 50: start = 100, the first minimizer is at 200: b = 200 - 100; raw = 968 - 468 - 100 = 400",
        ["ori++", "v_cut", "cut_no_path"], [[(400, 400)]],
        chain_case([_up("A") + [("C", p) for p in (200, 100, 300, 400, 500)]], loose=[("C", 50)], m=75))
    # the number of supporting assemblies and the truncation of their mean
    for name, steps, cuts, tags, mean in (
            ("support2_x.5", (1000, 1001), (), ["support2", "trunc.5"], "int(2001 / 2) = 1000"),
            ("support2_exact", (1000, 1002), (), ["support2"], "int(2002 / 2) = 1001"),
            ("support3_x.33", (1000, 1000, 1001), (), ["support3", "trunc.33"], "int(3001 / 3) = 1000"),
            ("support3_x.67", (1000, 1001, 1001), (), ["support3", "trunc.67"], "int(3002 / 3) = 1000"),
            ("support3_exact", (999, 1001, 1003), (), ["support3"], "int(3003 / 3) = 1001"),
            ("support2_of_3_x.5", (1000, 5000, 1003), (1,), ["support2", "trunc.5"], "the second reference is cut at the junction: int(2003 / 2) = 1001"),
            ("support1_of_3", (7000, 5000, 1003), (0, 1), ["support1"], "the first two references are cut at the junction: 1003")):
        dist = int(mean.split("= ")[-1]) if "=" in mean else int(mean.split(": ")[-1])
        raw = dist - 32 - 468 - 100
        add(name, f"A(+) C(+) whole, references {steps} apart; {mean}; raw = {dist} - 32 - 468 - 100 = {raw}", ["ori++"] + tags, [[(raw, raw)]],
            chain_case([_up("A") + _up("C")], refs=[dict(step=s, cuts={0: [5]} if r in cuts else {}) for r, s in enumerate(steps)]))
    # raw against g and G: A is L long, raw = 968 - (L - 532) - 100 = 1400 - L
    for name, L, g, G, gap, tags in (("raw_negative", 2000, 20, 0, 20, ["raw_negative"]), ("raw_negative_G", 2000, 20, 40, 20, ["raw_negative"]),
                                     ("raw_g-1", 1381, 20, 0, 20, ["raw_g-1"]), ("raw_g", 1380, 20, 0, 20, ["raw_g"]), ("raw_g+1", 1379, 20, 0, 21, ["raw_g+1"]),
                                     ("raw_G-1", 1361, 20, 40, 39, ["raw_G-1"]), ("raw_G", 1360, 20, 40, 40, ["raw_G"]), ("raw_G+1", 1359, 20, 40, 40, ["raw_G+1"]),
                                     ("raw_g1_0", 1400, 1, 0, 1, ["raw_g-1"]), ("raw_g1_1", 1399, 1, 0, 1, ["raw_g"]), ("raw_g1_2", 1398, 1, 0, 2, ["raw_g+1"]),
                                     ("raw_below_g_above_G", 1390, 50, 40, 40, [])):
        add(name, f"A(+) C(+) whole, A {L} long: a = {L} - 532, raw = 1400 - {L} = {1400 - L}; g = {g}, G = {G}: gap = {gap}", ["ori++"] + tags, [[(gap, 1400 - L)]],
            chain_case([_up("A") + _up("C")], lengths={"A": L}, g=g, G=G))
    # stretches through runs without an orientation; a second reference, 2000 apart, is cut at one edge of the stretch
    for edges, cut_at in ((2, 1), (63, 62), (64, 63), (64, 0), (65, 64), (300, 299), (300, 70)):
        n_b = edges - 1
        raw = 1000 * edges - 32 - 468 - 100
        add(f"stretch{edges}_cut{cut_at}", f"A(+) B(?) C(+), B of {n_b}: the stretch is {edges} edges, edge {cut_at} of it from the first reference alone: raw = {1000 * edges} - 32 - 468 - 100 = {raw}",
            ["ori++", f"stretch{edges}"] if edges != 2 else ["ori++"], [[(raw, raw)]],
            chain_case([_up("A") + _mixed("B", n_b) + _up("C")], refs=[{}, dict(step=2000, cuts={0: [5 + cut_at]})], lengths={"B": 10 * n_b + 100}))
    add("stretch_two_runs", "A(-) B(?) D(?) C(-), B of 3 and D of 4: 8 edges, one reference: raw = 8000 - 32 - 100 - 468 = 7400", ["ori--"], [[(7400, 7400)]],
        chain_case([_down("A") + _mixed("B", 3) + _mixed("D", 4, seed=1) + _down("C")]))
    # empty common support: three assemblies of weight 1, n = 1 (shape c of tests/test_gpu_format_paths.py)
    for g in (20, 3):
        add(f"empty_support_g{g}", f"A(+) X(?) C(+), X one minimizer; the edge in front of X is the first reference's alone, the one behind it the second's: gap = raw = g = {g}",
            ["ori++", "empty_support"], [[(g, g)]],
            chain_case([_up("A", 3) + [("X", 50)] + _up("C", 3, at=1100)], refs=[dict(cuts={0: [4]}), dict(cuts={0: [3]})], weights=[1.0, 1.0, 1.0], n=1, g=g,
                       lengths={"A": 400, "X": 100, "C": 2000}))
    # paths that end or begin in a run without an orientation, and paths of such runs only
    add("last_run_unoriented", "A(+) C(+) B(?): two nodes, raw = 400, C is the last node", ["ori++", "last_run_unoriented"], [[(400, 400)]],
        chain_case([_up("A") + _up("C") + _mixed("B", 5)]))
    add("first_and_last_run_unoriented", "B(?) A(-) C(+) D(?): raw = 968 - 100 - 100 = 768", ["ori-+", "last_run_unoriented"], [[(768, 768)]],
        chain_case([_mixed("B", 5) + _down("A") + _up("C") + [("D", 7)]]))
    add("only_unoriented", "four contigs of one minimizer each and one of mixed order: no node, an empty list", ["only_unoriented"], [[]],
        chain_case([[("P0", 77), ("P1", 77), ("P2", 77), ("P3", 77)] + _mixed("B", 5)]))
    add("only_unoriented_and_a_path", "path 0 as only_unoriented, path 1 A(+) C(-): raw = 968 - 468 - 468 = 32", ["only_unoriented", "ori+-"], [[], [(32, 32)]],
        chain_case([[("P0", 77), ("P1", 77)] + _mixed("B", 6), _up("A") + _down("C")]))
    add("single_node", "A(+) then one minimizer of C: one node, gap 0", ["last_run_unoriented"], [[]], chain_case([_up("A") + [("C", 5)]]))
    # a contig shorter than its minimizers imply: the reference raises ValueError
    add("a_negative", "path 0: A(+) C(+) with A 531 long: a = 531 - 500 - 32 = -1; path 1: D(+) E(+), raw = 400", ["ori++", "a_negative"], [None, [(400, 400)]],
        chain_case([_up("A") + _up("C"), _up("D") + _up("E")], lengths={"A": 531}))
    add("b_negative", "path 0: D(+) E(-), raw = 32; path 1: A(+) C(-) with C 531 long: b = 531 - 500 - 32 = -1", ["ori+-", "b_negative"], [[(32, 32)], None],
        chain_case([_up("D") + _down("E"), _up("A") + _down("C")], lengths={"C": 531}))
    return t


def gaps_case(name):
    doc, tags, expect, case = _gap_table()[name]
    return dict(case, doc=doc, tags=list(tags), expect=expect)


# -- wide
@functools.lru_cache(maxsize=None)
def wide_case(n_paths=1500, seed=7):
    """n_paths paths of three target contigs each, 2 to 70 minimizers long, increasing, decreasing (one pair in twenty-odd out of
    order in some) or mixed, whole or cut by a vertex on no path below or above; two references of weight 2, the second cut
    into up to four records per path, and both lacking a few minimizers, which then are no vertices.  Cached: read it, do not
    change it"""
    rng = random.Random(seed)
    r0, r1, target, lengths, lone = [], [], [], {}, []
    nh = [0]

    def new_hash():
        nh[0] += 1
        return nh[0] * 2_654_435_761 % (1 << 61) + 1

    for p in range(n_paths):
        chain = []
        for c in range(3):
            ctg, ori = f"p{p}c{c}", rng.choice("+-?")
            n = rng.randint(3 if ori == "?" else 2, 70)
            pos = [60 + 37 * i + rng.randrange(20) for i in range(n)]
            if ori == "?":
                pos = _shuffle_mixed(rng, pos)
            else:
                if n >= 22 and rng.random() < 0.3:
                    i = rng.randrange(1, n - 2)
                    pos[i], pos[i + 1] = pos[i + 1], pos[i]
                if ori == "-":
                    pos.reverse()
            mxs = [(new_hash(), q) for q in pos]
            chain += mxs
            cut = rng.choice(["whole", "whole", "low", "high", "both"])
            hi, own = max(pos), []
            if cut in ("low", "both"):
                own.append((new_hash(), 10 + rng.randrange(40)))
            if cut in ("high", "both"):
                hi += 100 + rng.randrange(200)
                own.append((new_hash(), hi))
            lone += [h for h, _q in own]
            lengths[ctg] = hi + K + rng.randrange(60)
            target.append((ctg, mxs + own))
        at0 = at1 = 0
        rec0, recs1 = [], [[]]
        cuts = set(rng.sample(range(1, len(chain)), rng.randint(0, 3)))
        for i, (h, _q) in enumerate(chain):
            at0 += rng.randint(500, 1500)
            at1 += rng.randint(500, 1500)
            if i in cuts:
                recs1.append([])
            if rng.random() >= 0.03:
                rec0.append((h, at0))
            if rng.random() >= 0.03:
                recs1[-1].append((h, at1))
        r0.append((f"chr{p}", rec0))
        r1 += [(f"alt{p}.{j}", rec) for j, rec in enumerate(recs1) if rec]
    for j, h in enumerate(lone):
        r0.append((f"lone{j}", [(h, 1000)]))
        r1.append((f"lone{j}", [(h, 2000)]))
    return dict(asms=[r0, r1, target], weights=[2.0, 2.0, 1.0], lengths=lengths, k=K, n=2, g=20, G=0, m=90)


def _shuffle_mixed(rng, pos):
    "pos in an order in which fewer than 75 % of the consecutive pairs increase and fewer than 75 % decrease"
    assert len(pos) != 2
    while len(pos) > 1:
        out = list(pos)
        rng.shuffle(out)
        inc = sum(a < b for a, b in zip(out, out[1:]))
        if 4 * max(inc, len(out) - 1 - inc) < 3 * (len(out) - 1):
            return out
    return list(pos)


# ---- families: inputs re-made here, the reference's answers under tests/golden/format/families --------------------------------------
GENERATORS = {"fuzz_case": fuzz_case, "m_rule_case": m_rule_case, "gaps_case": gaps_case, "wide_case": wide_case}
WIDE_HEAD = 50   # paths of the wide case that its golden holds verbatim
FAMILIES = ("fuzz", "m_rule", "gaps", "wide")


def family_specs():
    "family -> [(case name, generator, arguments)]: what make_golden_format.py records and the tests read back"
    return {
        "fuzz": [(f"draw{i:02d}", "fuzz_case", dict(i=i)) for i in range(FUZZ_CASES)],
        "m_rule": _m_rule_specs(),
        "gaps": [(name, "gaps_case", dict(name=name)) for name in _gap_table()],
        "wide": [("wide", "wide_case", {})],
    }


def case_input(case):
    return [case["asms"], case["weights"], case["lengths"], case["k"], case["n"], case["g"], case["G"], case["m"]]


def json_digest(value):
    return hashlib.sha256(json.dumps(value, separators=(",", ":")).encode("ascii")).hexdigest()


def case_digest(case):
    return json_digest(case_input(case))


def universe(case):
    "the case's hashes in ascending order: paths and rows are recorded with a minimizer's index into it"
    return sorted({h for asm in case["asms"] for _rid, mxs in asm for h, _pos in mxs})


def asm_names(case):
    return [f"r{a}" for a in range(len(case["asms"]) - 1)] + ["t"]


def write_tsvs(case, directory):
    "the assemblies as minimizer TSVs (record<TAB>hash:pos:seq ...), sorted by position within a record -> their paths, target last"
    paths = []
    for name, asm in zip(asm_names(case), case["asms"]):
        paths.append(os.path.join(directory, name + ".tsv"))
        with open(paths[-1], "w", encoding="ascii") as fh:
            for rid, mxs in asm:
                fh.write(rid + "\t" + " ".join(f"{h}:{p}:A" for h, p in sorted(mxs, key=lambda hp: hp[1])) + "\n")
    return paths


def pack(case, paths, rows):
    """paths (lists of hash strings) and the rows of each -> (paths, rows) with hashes as universe indexes, the paths in ascending
    order of those lists (the reference's own order follows python's set order) and the rows in the order of their paths"""
    index = {str(h): i for i, h in enumerate(universe(case))}
    packed = sorted(([index[v] for v in path], None if nodes is None else [r[:5] + [index[r[5]], index[r[6]]] + r[7:] for r in nodes])
                    for path, nodes in zip(paths, rows))
    return [p for p, _r in packed], [r for _p, r in packed]


def unpack(case, paths, rows):
    "-> (paths as tuples of hashes, rows with the hashes as decimal strings, as format_paths gives them)"
    uni = universe(case)
    return ([tuple(uni[i] for i in path) for path in paths],
            [None if nodes is None else [r[:5] + [str(uni[r[5]]), str(uni[r[6]])] + r[7:] for r in nodes] for nodes in rows])


def summarise_wide(paths, rows):
    "what the wide case's golden holds in place of its packed paths and rows"
    assert all(len(nodes) <= 9 for nodes in rows)   # counts: one digit per path
    return dict(paths_sha256=json_digest(paths), rows_sha256=json_digest(rows), counts="".join(str(len(nodes)) for nodes in rows),
                n_paths=len(paths), paths_head=paths[:WIDE_HEAD], rows_head=rows[:WIDE_HEAD])


@functools.lru_cache(maxsize=None)
def load_family(family):
    """-> {case name: golden entry with "case" (the input, re-made and checked against the recorded digest) and, but for the wide
    case, "paths" and "rows" unpacked to hashes (rows None where "error" names the path)}.  Cached: read it, do not change it"""
    with open(os.path.join(GOLDEN, "families", family + ".json"), encoding="ascii") as fh:
        doc = json.load(fh)
    out = {}
    for entry in doc["cases"]:
        meta = entry["meta"]
        case = GENERATORS[meta["generator"]](**meta["args"])
        assert case_digest(case) == meta["sha256"], f"{family}/{meta['name']}: the generator no longer gives the input the golden was recorded on"
        entry = dict(entry, case=case)
        if "paths" in entry:
            entry["paths"], entry["rows"] = unpack(case, entry["paths"], entry["rows"])
        out[meta["name"]] = entry
    assert list(out) == [name for name, _g, _a in family_specs()[family]], f"{family}: the golden's cases are not those of family_specs()"
    return out


# ---- what a recorded answer holds: the counts behind the conditions of tests/golden/format/README.md -------------------------------
def fuzz_counts(entries):
    """over the fuzz goldens, from the reference's own answers and the inputs: paths, nodes (rows), runs of two or more minimizers
    that are not strictly monotone, errors, junctions over more than one edge, with empty support, G-capped"""
    c = dict(paths=0, nodes=0, not_monotone=0, errors=0, long_stretch=0, empty_support=0, capped=0)
    for entry in entries.values():
        case = entry["case"]
        where = {h: (rid, pos) for rid, mxs in case["asms"][-1] for h, pos in mxs}
        c["errors"] += "error" in entry
        support = _edge_support(case)
        for path, nodes in zip(entry["paths"], entry["rows"]):
            c["paths"] += 1
            c["nodes"] += len(nodes)
            runs = []
            for h in path:
                rid, pos = where[h]
                if runs and runs[-1][0] == rid:
                    runs[-1][1].append(pos)
                else:
                    runs.append((rid, [pos]))
            for _rid, pos in runs:
                pairs = list(zip(pos, pos[1:]))
                c["not_monotone"] += len(pos) > 1 and not (all(a < b for a, b in pairs) or all(a > b for a, b in pairs))
            at = {h: i for i, h in enumerate(path)}
            for u, v in zip(nodes or [], (nodes or [])[1:]):
                iu, iv = at[int(u[6])], at[int(v[5])]
                c["long_stretch"] += iv - iu > 1
                common = set.intersection(*[support[frozenset(e)] for e in zip(path[iu:iv], path[iu + 1:iv + 1])])
                c["empty_support"] += not common
                if not common:
                    assert u[7] == u[8] == case["g"]
                c["capped"] += case["G"] > 0 and u[8] > case["G"] and u[7] == case["G"]
    return c


def _edge_support(case):
    "edge -> the assemblies that hold its two minimizers next to each other, among the minimizers that all assemblies hold"
    shared = set.intersection(*[{h for _rid, mxs in asm for h, _pos in mxs} for asm in case["asms"]])
    support = {}
    for a, asm in enumerate(case["asms"]):
        for _rid, mxs in asm:
            kept = [h for h, _pos in sorted(mxs, key=lambda hp: hp[1]) if h in shared]
            for e in zip(kept, kept[1:]):
                support.setdefault(frozenset(e), set()).add(a)
    return support


FUZZ_MINIMUMS = dict(paths=100, nodes=500, not_monotone=150, long_stretch=40, empty_support=1, capped=20)


def check_conditions(family, entries):
    "the conditions that keep the pin from going hollow, from the recorded answers; -> the counts (fuzz) or tags (gaps) found"
    if family == "fuzz":
        counts = fuzz_counts(entries)
        assert counts["errors"] == 0, counts
        for name, least in FUZZ_MINIMUMS.items():
            assert counts[name] >= least, (name, counts)
        return counts
    if family == "m_rule":
        for inc, d, m, want in M_RULE_FLOAT:
            entry = entries[f"float_{inc}_{d}_m{m}"]
            assert entry["case"]["u_pairs"] == [d + 1, inc, d - inc]
            assert u_orientation(entry) == want, (inc, d, m, u_orientation(entry))
        return {name: u_orientation(entry) for name, entry in entries.items()}
    if family == "gaps":
        seen = set()
        for name, entry in entries.items():
            case = entry["case"]
            seen.update(case["tags"])
            raised = [p for p, nodes in enumerate(entry["rows"]) if nodes is None]
            assert raised == ([entry["error"]["path"]] if "error" in entry else []), name
            assert ("a_negative" in case["tags"] or "b_negative" in case["tags"]) == ("error" in entry), name
            # the chains are walked upwards, so path p of the generator is path p in ascending order of the hash indexes
            got = [None if nodes is None else [(r[7], r[8]) for r in nodes[:-1]] for nodes in entry["rows"]]
            assert got == [None if e is None else [tuple(x) for x in e] for e in case["expect"]], (name, got, case["expect"])
            assert all(nodes[-1][7:] == [0, 0] for nodes in entry["rows"] if nodes)
        assert seen == set(GAP_TAGS), set(GAP_TAGS) - seen
        assert sum("error" in entry for entry in entries.values()) == 2
        return sorted(seen)
    assert family == "wide"
    entry = entries["wide"]
    counts = dict(paths=entry["n_paths"], nodes=sum(map(int, entry["counts"])))
    assert counts["paths"] >= 1500 and len(entry["counts"]) == counts["paths"] and "error" not in entry
    return counts


def u_orientation(entry):
    "the recorded orientation of contig U of an m_rule case ('?': the reference made no node of it)"
    oris = [r[1] for nodes in entry["rows"] for r in nodes if r[0] == "U"]
    assert len(entry["rows"]) == 1 and len(oris) <= 1
    return oris[0] if oris else "?"
