"""Piece tables for the tests of mxg_compose_pieces (tests/test_compose_cpu.py, tests/test_gpu_compose.py): the hand-made cases, the
seeded fuzz, the refusals, and the invariant every composition must keep: a record spells the same sequence before and after."""
import random

from tests import _compose_restatement as R

F, V, G = R.FWD, R.REV, R.GAP
BASE_LEN = [500, 500, 500, 500]   # the contigs the hand-made inner table is cut from

# record 1: pieces at 0, 50, 70, 130, 135 of its 175 bases
INNER = [
    [(0, 10, 110, F)],
    [(1, 0, 50, F), (0, 0, 20, G), (2, 100, 160, V), (0, 0, 5, G), (3, 7, 47, F)],
    [(2, 0, 30, V), (0, 0, 10, G)],
]

# name -> outer table over INNER
HAND = {
    "equal_to_one_inner_piece": [[(1, 70, 130, F)], [(1, 70, 130, V)], [(1, 50, 70, F)]],
    "strictly_inside_one_inner_piece": [[(1, 80, 120, F)], [(1, 80, 120, V)], [(1, 55, 60, V)], [(0, 1, 99, F)]],
    "ending_on_inner_borders": [[(1, 50, 135, F)], [(1, 0, 50, F)], [(1, 135, 175, V)], [(1, 50, 135, V)]],
    "across_mixed_pieces": [[(1, 10, 150, F)], [(1, 0, 175, F)], [(1, 49, 136, F)]],
    "rev_over_fwd_rev_gap": [[(1, 10, 150, V)], [(1, 0, 175, V)], [(2, 0, 40, V)], [(2, 29, 31, V)]],
    "cut_in_gap_next_to_outer_gap": [
        [(1, 0, 60, F), (0, 0, 15, G), (1, 65, 175, F)],      # 50 bases, then 10 + 15 + 5 Ns as ONE gap
        [(1, 60, 175, V), (0, 0, 15, G), (1, 0, 55, V)],
        [(2, 0, 40, F), (0, 0, 3, G), (0, 0, 4, G), (1, 50, 60, F), (1, 60, 70, V), (2, 30, 40, V), (0, 5, 95, F)],
        [(1, 130, 135, F), (1, 130, 135, V)],                   # a record that becomes one gap
    ],
    "record_of_one_piece": [[(0, 0, 100, F)], [(0, 0, 100, V)], [(0, 0, 1, F)], [(0, 0, 7, G)]],
    "several_records": [[(0, 0, 100, F), (0, 0, 9, G), (1, 20, 80, V)], [(2, 10, 35, F)], [(1, 0, 175, F), (1, 0, 175, V)]],
}

# name -> (inner, outer, code)
REFUSED = {
    "outer_beyond_inner_record": (INNER, [[(1, 100, 176, F)]], R.EINVAL),
    "outer_beyond_inner_record_rev": (INNER, [[(0, 0, 100, F)], [(2, 39, 41, V)]], R.EINVAL),
    "outer_names_no_inner_record": (INNER, [[(3, 0, 1, F)]], R.EINVAL),
    "inner_record_without_pieces": ([INNER[0], [], INNER[2]], [[(0, 0, 100, F)]], R.EINVAL),
    "outer_record_without_pieces": (INNER, [[(0, 0, 100, F)], []], R.EINVAL),
    "empty_outer_piece": (INNER, [[(0, 5, 5, F)]], R.EINVAL),
    "inverted_inner_piece": ([[(0, 9, 3, V)]], [[(0, 0, 1, F)]], R.EINVAL),
    "unknown_kind": (INNER, [[(0, 0, 10, 3)]], R.EINVAL),
    "inner_record_of_2_32_bases": ([[(0, 0, 2 ** 31, G), (0, 0, 2 ** 31, G)]], [[(0, 0, 1, F)]], R.ELIMIT),
}


def flatten(table):
    "-> (rows of four numbers, n_records + 1 offsets)"
    rows, first = [], [0]
    for rec in table:
        rows.extend(rec)
        first.append(len(rows))
    return rows, first


def unflatten(rows, first):
    rows = [tuple(int(x) for x in row) for row in rows]
    return [rows[int(first[r]):int(first[r + 1])] for r in range(len(first) - 1)]


def random_table(rng, n_records, ref_len, max_pieces=8, gap_p=0.25):
    "a valid table over records of the lengths ref_len; neighbouring gaps do occur"
    table = []
    for _ in range(n_records):
        rec = []
        for _ in range(rng.randint(1, max_pieces)):
            if rng.random() < gap_p:
                rec.append((0, 0, rng.randint(1, 40), G))
            else:
                r = rng.randrange(len(ref_len))
                a = rng.randrange(ref_len[r])
                b = rng.choice((ref_len[r], a + 1, rng.randint(a + 1, ref_len[r])))
                rec.append((r, a, b, rng.choice((F, V))))
        table.append(rec)
    return table


def fuzz_case(seed, n_outer=None, inner_pieces=None, outer_pieces=4):
    """-> (base_len, inner, outer).  inner_pieces: every inner record has exactly that many pieces; outer_pieces: the most an outer
    record has"""
    rng = random.Random(seed)
    base_len = [rng.randint(1, 300) for _ in range(rng.randint(1, 6))]
    inner = random_table(rng, rng.randint(1, 7), base_len)
    if inner_pieces:
        inner = [(rec * inner_pieces)[:inner_pieces] for rec in inner]
    inner_len = [R.record_length(rec) for rec in inner]
    outer = random_table(rng, n_outer if n_outer is not None else rng.randint(1, 9), inner_len, max_pieces=outer_pieces)
    return base_len, inner, outer


def check_spelling(base_len, inner, outer, result, seed=0):
    "every outer record spells over the inner records' spelling what its result spells over the base records"
    rng = random.Random(seed)
    base = ["".join(rng.choice("ACGTNacgtRYKMn") for _ in range(n)) for n in base_len]
    mid = [R.spell(rec, base) for rec in inner]
    assert len(result) == len(outer)
    for r, (rec, res) in enumerate(zip(outer, result)):
        assert R.spell(res, base) == R.spell(rec, mid), r
        assert res and all(s < e for _, s, e, _ in res), r
        assert not any(x[3] == G and y[3] == G for x, y in zip(res, res[1:])), f"record {r}: two gaps in a row"
        assert all((q[0], q[1]) == (0, 0) for q in res if q[3] == G), r
