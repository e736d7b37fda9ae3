"""CPU tests of the path adjustment stage's test infrastructure: the restatement (tests/_adjust_restatement.py) against every
golden recorded from the reference's own functions (tests/golden/adjust), the pybedtools stand-in the goldens were made with
against a brute-force count, the hand-made cases against what the goldens hold, what the seeded fuzz cases cover, and the
restatement against the families recorded from the reference on the seeded inputs (fuzz, ladder, strided, large)."""
import collections
import glob
import os
import random
import sys

import pytest

from tests import _adjust_cases as cases, _adjust_restatement as rs

GOLDENS = cases.load_goldens()


def test_goldens_are_all_there():
    hand = {"hand_" + name for name in cases.hand_cases()}
    assert hand <= set(GOLDENS) and len(GOLDENS) == len(hand) + 5
    for name, case in cases.hand_cases().items():
        doc = GOLDENS["hand_" + name]
        assert (doc["paths"], doc["no_cut"], doc["G"]) == (case["paths"], case["no_cut"], case["G"]), name
    specs = cases.family_specs()
    files = sorted(os.path.basename(f) for f in glob.glob(os.path.join(cases.GOLDEN, "families", "*")))
    assert files == sorted(family + ".json" for family in specs) == ["fuzz.json", "ladder.json", "large.json", "strided.json"]
    assert {family: len(spec) for family, spec in specs.items()} == {"fuzz": 200, "ladder": 23, "strided": 2, "large": 1}
    for family, spec in specs.items():
        docs = cases.load_family(family)
        assert list(docs) == [name for name, _g, _a in spec], family
        for name, generator, args in spec:
            assert (docs[name]["meta"]["generator"], docs[name]["meta"]["args"]) == (generator, args), (family, name)


@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_restatement_equals_golden(name):
    doc = GOLDENS[name]
    result, source = rs.adjust(doc["paths"], doc["no_cut"], doc["G"])
    assert result == doc["result"]
    assert [[list(w) for w in path] for path in source] == doc["source"]


def test_hand_cases_keep_the_tie_rule_out():
    "no two overlapping segments of one contig with equal start in the sets whose intersections are counted"
    for name, doc in GOLDENS.items():
        trace = {}
        rs.adjust(doc["paths"], doc["no_cut"], doc["G"], trace)
        for contig, group in trace["sets"].items():
            for a in group:
                for b in group:
                    assert a == b or a[0] != b[0] or not rs.intersects(a, b), (name, contig, a, b)


def test_no_cut_golden_is_the_path_the_reference_pins():
    doc = GOLDENS["regions-ff-rr_n1_no_cut"]
    kept = [path for path in doc["result"] if len(path) >= 2]
    assert len(kept) == 1
    assert " ".join(f"{c}{o}:{s}-{e} {g}N" for c, o, s, e, _n, _f, _t, g, _r in kept[0]) == "2_1n-1_2p-:0-4379 20N 1_1p-2_2n-:0-4489 0N"


def test_duplicate_segment_raises_keyerror():
    case = cases.duplicate_case()
    with pytest.raises(KeyError) as err:
        rs.adjust(case["paths"], case["no_cut"], case["G"])
    assert err.value.args[0] == (1, 1)


def test_standin_counts_equal_brute_force():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    try:
        import pybedtools_standin as pb
    finally:
        sys.path.pop(0)
    rng = random.Random(11)
    for _ in range(200):
        rows = set()
        for _n in range(rng.randint(0, 40)):
            start = rng.randint(0, 60)
            rows.add((rng.choice(["a", "b", "c10", "c9"]), start, start + rng.randint(1, 25)))
        rows = list(rows)
        rng.shuffle(rows)
        bed = pb.BedTool("\n".join(f"{c}\t{s}\t{e}" for c, s, e in rows), from_string=True).sort()
        got = [(iv.chrom, iv.start, iv.end, iv.count) for iv in bed.intersect(b=bed, c=True, wa=True)]
        want = [(c, s, e, sum(1 for c2, s2, e2 in rows if c2 == c and max(s, s2) < min(e, e2))) for c, s, e in sorted(rows)]
        assert got == want
        for contig in {r[0] for r in rows}:  # ... and the restatement counts the same
            segs = [(s, e) for c, s, e in rows if c == contig]
            assert rs.intersection_counts(segs) == [((s, e), n) for c, s, e, n in want if c == contig]


def test_fuzz_covers_merges_blocks_and_overlaps():
    seen, errors = collections.Counter(), 0
    for seed in cases.FUZZ_SEEDS:
        case = cases.fuzz_case(seed)
        assert len(case["paths"]) <= 40 and all(1 <= len(p) <= 8 for p in case["paths"])
        assert len({row[0] for p in case["paths"] for row in p}) <= 12
        try:
            result, source = rs.adjust(case["paths"], case["no_cut"], case["G"])
        except KeyError:
            errors += 1
            continue
        seen.update(cases.features(case, result, source))
    for feature in ("merge", "blocked", "overlap", "overlap_cut", "dropped"):
        assert seen[feature] >= len(cases.FUZZ_SEEDS) // 10, (feature, seen)
    assert 0 < errors <= len(cases.FUZZ_SEEDS) // 10


# ---- the families: seeded inputs, the reference's recorded answers ------------------------------------------------------------------
FAMILY_CASES = [(family, name) for family, spec in cases.family_specs().items() for name, _g, _a in spec]
# fuzz seeds whose answer changes with the order of two segments of equal start (README.md of the goldens); all are no_cut=False
TIE_DEPENDENT = [14, 26, 28, 34, 46, 58, 64, 78, 84, 90, 100, 102, 104, 118, 136, 144, 148, 156, 160, 164, 170]
ERROR_SEEDS = [0, 56, 98, 168]


def test_every_generated_case_is_one_ntjoin_could_see():
    for case in cases.hand_cases().values():
        cases.check_case(case)
    for doc in GOLDENS.values():
        cases.check_case(doc)
    cases.check_case(cases.duplicate_case())
    for spec in cases.family_specs().values():
        for _name, generator, args in spec:
            cases.check_case(cases.GENERATORS[generator](**args))
    with pytest.raises(AssertionError):  # the guard sees what it is there for: one contig under two sizes
        cases.check_case(dict(paths=[[["m", "+", 0, 50, 50, "1", "2", 0, 0]], [["m", "-", 60, 90, 100, "3", "4", 0, 0]]]))
    for bad in (["m", "+", 5, 5, 50, "1", "2", 0, 0], ["m", "+", 0, 51, 50, "1", "2", 0, 0], ["m", "*", 0, 50, 50, "1", "2", 0, 0]):
        with pytest.raises(AssertionError):
            cases.check_case(dict(paths=[[bad]]))


def test_recorded_digests_equal_the_regenerated_inputs():
    "load_family asserts each digest; here also that it is the digest of what the generator gives now, under the recorded arguments"
    for family, spec in cases.family_specs().items():
        docs = cases.load_family(family)
        for name, generator, args in spec:
            assert docs[name]["meta"]["sha256"] == cases.case_digest(cases.GENERATORS[generator](**args)), (family, name)
            assert docs[name]["case"] == cases.GENERATORS[generator](**args), (family, name)


@pytest.mark.parametrize("family,name", FAMILY_CASES, ids=[f"{f}-{n}" for f, n in FAMILY_CASES])
def test_restatement_equals_family_golden(family, name):
    doc = cases.load_family(family)[name]
    case = doc["case"]
    if "error" in doc:
        with pytest.raises(KeyError) as err:
            rs.adjust(case["paths"], case["no_cut"], case["G"])
        p, i = err.value.args[0]
        assert p == doc["error"]["path"]
        assert case["paths"][p][i][0] == doc["error"]["contig"]
        return
    result, source = case.get("expected") or rs.adjust(case["paths"], case["no_cut"], case["G"])
    source = [[list(w) for w in path] for path in source]
    if family == "large":
        got = cases.summarise_large(result, source)
        assert got["result_head"] == doc["result_head"] and got["source_head"] == doc["source_head"]
        assert got["counts"] == doc["counts"]
        assert (got["result_sha256"], got["source_sha256"]) == (doc["result_sha256"], doc["source_sha256"])
        return
    assert result == doc["result"]
    assert source == doc["source"]


def test_tie_dependent_seeds_are_the_listed_ones():
    fuzz = cases.load_family("fuzz")
    tied = [seed for seed in cases.FUZZ_SEEDS if not fuzz[f"seed{seed:03d}"]["meta"]["tie_independent"]]
    assert tied == TIE_DEPENDENT
    assert len(tied) <= 30  # 21 measured; beyond 30 the fuzz would be sliding onto the rule that no golden pins
    assert all(not cases.fuzz_case(seed)["no_cut"] for seed in tied)
    assert [seed for seed in cases.FUZZ_SEEDS if "error" in fuzz[f"seed{seed:03d}"]] == ERROR_SEEDS
    for family in ("ladder", "strided", "large"):
        for name, doc in cases.load_family(family).items():
            assert doc["meta"]["tie_independent"], (family, name)


def test_ladder_has_every_outcome_at_every_length():
    ladder = cases.load_family("ladder")
    assert cases.LADDER_L == [2, 3, 63, 64, 65, 127, 128, 129, 200, 257]
    for L in cases.LADDER_L:
        for no_cut in (False, True):
            doc = ladder[f"L{L}" + ("_no_cut" if no_cut else "")]
            case = doc["case"]
            assert case["no_cut"] == no_cut
            per_contig = collections.Counter(row[0] for path in case["paths"] for row in path)
            assert per_contig["X"] == L and per_contig["Y"] == L, (L, no_cut)
            assert all(len(path) >= 2 for path in case["paths"])
            starts = [row[2] for path in case["paths"] for row in path if row[0] == "X"]
            assert len(set(starts)) == L  # the order of equal starts stays out
            assert len({row[2] for path in case["paths"] for row in path if row[0] == "Y"}) == L
            last = [row for row in case["paths"][-1] if row[0] == "Y"]  # the last of Y's list shares bases with exactly one other
            assert len(last) == 1 and sum(rs.intersects(last[0][2:4], row[2:4]) for path in case["paths"] for row in path if row[0] == "Y") == 2
            if L >= 63 and not no_cut:
                source = [[tuple(w) for w in path] for path in doc["source"]]
                assert cases.features(case, doc["result"], source) == {"merge", "blocked", "overlap", "overlap_cut", "dropped"}, L
    assert [len(ladder[f"paths{P}"]["case"]["paths"]) for P, _n in cases.LADDER_PATHS] == [255, 256, 257]
    assert [ladder[f"paths{P}"]["case"]["no_cut"] for P, _n in cases.LADDER_PATHS] == [False, True, False]


def test_strided_case_keeps_its_lists():
    for no_cut in (False, True):
        case = cases.strided_case(no_cut)
        per_contig = collections.Counter(row[0] for path in case["paths"] for row in path)
        assert per_contig["BIG"] == 200 and per_contig["CH"] == 70 and per_contig["MIX"] > 64
    chain = [row for path in cases.load_family("strided")["strided"]["result"] for row in path if row[0] == "CH"]
    assert len(chain) == 1 and (chain[0][2], chain[0][3]) == (0, 6960)
