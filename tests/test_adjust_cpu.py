"""CPU tests of the path adjustment stage's test infrastructure: the restatement (tests/_adjust_restatement.py) against every
golden recorded from the reference's own functions (tests/golden/adjust), the pybedtools stand-in the goldens were made with
against a brute-force count, the hand-made cases against what the goldens hold, and what the seeded fuzz cases cover."""
import collections
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
