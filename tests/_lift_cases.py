"""Tables, features and BED text for the tests of mxg_lift_prepare / mxg_lift_intervals / mxg_lift_bed (tests/test_lift_cpu.py,
tests/test_gpu_lift.py): the hand-made cases, the seeded fuzz, the refusals, and the property every lift must keep: a part spells in
the scaffold what its stretch of the feature spells in the source record, reverse-complemented when `reverse`."""
import functools
import random

from tests import _compose_cases as CC, _compose_restatement as C, _lift_restatement as R

F, V, G = R.FWD, R.REV, R.GAP

# ctg0 is cut at 400 and its halves go to two scaffolds; ctg1 loses [0, 50) and [450, 500) and is reversed; no piece names ctg3;
# ctg4 lies whole in record 2, and a short stretch of it, which starts later and ends earlier, once more in record 3; the last
# source record has the name of ctg1 over again
SOURCE_LEN = [1000, 500, 300, 200, 300, 77]
SOURCE_NAMES = [b"ctg0", b"ctg1", b"ctg2", b"ctg3", b"ctg4", b"ctg1"]
TABLE = [
    [(0, 0, 400, F), (0, 0, 20, G), (1, 50, 450, V)],
    [(0, 400, 1000, F), (0, 0, 5, G), (2, 0, 300, V)],
    [(4, 0, 300, F)],
    [(0, 0, 9, G), (4, 100, 150, V)],
]
SCAFFOLD_NAMES = [b"ntJoin0", b"ntJoin1", b"ctg4:0-300", b"ntJoin3"]

# name -> (feature, status, parts), worked by hand
HAND = {
    "inside_one_fwd_piece": ((0, 10, 50), R.WHOLE, [(0, 10, 50, 10, 0)]),
    "inside_one_rev_piece": ((1, 100, 200), R.WHOLE, [(0, 670, 770, 100, 1)]),          # 420 + (450 - 200), 420 + (450 - 100)
    "ending_at_a_piece_end": ((0, 300, 400), R.WHOLE, [(0, 300, 400, 300, 0)]),
    "starting_at_a_piece_end": ((0, 400, 410), R.WHOLE, [(1, 0, 10, 400, 0)]),
    "across_a_cut_between_scaffolds": ((0, 350, 500), R.SPLIT, [(0, 350, 400, 350, 0), (1, 0, 100, 400, 0)]),
    "over_a_trimmed_stretch": ((1, 0, 100), R.PARTIAL, [(0, 770, 820, 50, 1)]),
    "over_both_trimmed_stretches": ((1, 0, 500), R.PARTIAL, [(0, 420, 820, 50, 1)]),
    "inside_a_trimmed_stretch": ((1, 10, 40), R.LOST, []),
    "behind_the_last_piece": ((1, 450, 500), R.LOST, []),
    "record_no_piece_names": ((3, 0, 200), R.LOST, []),
    "behind_a_nested_short_piece": ((4, 200, 250), R.WHOLE, [(2, 200, 250, 200, 0)]),
    "same_base_in_two_pieces": ((4, 120, 130), R.SPLIT, [(2, 120, 130, 120, 0), (3, 29, 39, 120, 1)]),   # 9 + (150 - 130)
    "over_the_nested_piece_and_beyond": ((4, 90, 160), R.SPLIT, [(2, 90, 160, 90, 0), (3, 9, 59, 100, 1)]),
    "whole_record_reversed": ((2, 0, 300), R.WHOLE, [(1, 605, 905, 0, 1)]),
    "one_base": ((0, 999, 1000), R.WHOLE, [(1, 599, 600, 999, 0)]),
    "empty": ((0, 5, 5), R.INVALID, []),
    "inverted": ((0, 7, 3), R.INVALID, []),
    "past_the_record": ((0, 990, 1001), R.INVALID, []),
    "record_out_of_range": ((6, 0, 10), R.INVALID, []),
    "record_2_32_less_1": ((2 ** 32 - 1, 0, 10), R.INVALID, []),
}

BED = b"".join([
    b"track name=genes\n",
    b"# a comment\n",
    b"browser position ctg0:1-100\n",
    b"ctg0\t10\t50\n",                                                       # 3 columns
    b"ctg0\t10\t50\tgeneA\n",                                                # 4
    b"ctg1\t100\t200\tgeneB\t0\t+\n",                                        # 6, on a reverse piece: flipped
    b"ctg1\t100\t200\tgeneB\t0\t-\n",
    b"ctg1\t100\t200\tgeneC\t0\t.\n",
    b"ctg1\t100\t200\tgeneD\t960\t+\t120\t180\t0,0,255\t2\t10,20\t0,80\n",   # 12
    b"ctg0\t350\t500\tsplit\t0\t+\r\n",
    b"ctg1\t0\t100\tpartial\n",
    b"ctg1\t10\t40\tlost\n",
    b"ctg0\t12345678901\t5\televen_digits\n",
    b"ctg0\t4294967296\t4294967297\ttoo_large\n",
    b"ctg0\t1x\t5\n",
    b"ctg0\t 1\t5\n",
    b"ctg0\t\t5\n",
    b"ctg0\t5\n",
    b"ctg0\n",
    b"\t1\t2\tempty_name\n",
    b"nope\t1\t2\tunknown\n",
    b"nope\t2\t1\tunknown_and_inverted\n",
    b"ctg4\t120\t130\ttwice\t0\t-\n",
    b"ctg4\t200\t250\tnested\n",
    b"\n",
    b"\r\n",
    b"ctg1\t100\t200\tgeneE\t0\t++\n",
    b"ctg1\t100\t200\tgeneF\t0\t-\r\n",
    b"ctg0\t10\t50\t\n",                                                     # an empty column 4
    b"ctg0 \t10\t50\tname_with_blank\n",
    b"ctg3\t0\t200\tno_piece\n",
    b"tracked\t0\t1\n",                                                      # begins with "track"
    b"ctg2\t0\t300\tlast\t0\t-",                                             # no final newline
])

# name -> (table, source_length, code)
REFUSED = {
    "piece_beyond_its_source_record": ([[(0, 0, 400, F)], [(1, 0, 501, V)]], SOURCE_LEN, R.EINVAL),
    "piece_names_no_source_record": ([[(0, 0, 400, F), (6, 0, 1, F)]], SOURCE_LEN, R.EINVAL),
    "record_without_pieces": ([[(0, 0, 400, F)], []], SOURCE_LEN, R.EINVAL),
    "empty_piece": ([[(0, 5, 5, F)]], SOURCE_LEN, R.EINVAL),
    "unknown_kind": ([[(0, 0, 10, 3)]], SOURCE_LEN, R.EINVAL),
    "record_of_2_32_bases": ([[(0, 0, 2 ** 31, G), (0, 0, 2 ** 31, G)]], SOURCE_LEN, R.ELIMIT),
}


def complement(s):
    return s[::-1].translate(C.COMP)


def sources(source_length, seed=0):
    rng = random.Random(seed)
    return ["".join(rng.choice("ACGTNacgtRYKMn") for _ in range(n)) for n in source_length]


def check_spelling(table, source_length, features, statuses, part_first, parts, seed=0, whole_only=False):
    """every part spells in its scaffold what its stretch of the feature spells in the source; the parts of a feature are in order
    and inside it; the status follows from them"""
    src = sources(source_length, seed)
    scaf = [C.spell(rec, src) for rec in table]
    assert len(statuses) == len(features) and len(part_first) == len(features) + 1 and part_first[0] == 0 and part_first[-1] == len(parts)
    for i, (r, a, b) in enumerate(features):
        mine = parts[part_first[i]:part_first[i + 1]]
        if statuses[i] in (R.INVALID, R.UNKNOWN, R.LOST) or (whole_only and statuses[i] != R.WHOLE):
            assert not mine, i
            continue
        lifted = 0
        for R_, s, e, lo, rev in mine:
            n = e - s
            assert n > 0 and a <= lo and lo + n <= b, i
            want = src[r][lo:lo + n]
            assert scaf[R_][s:e] == (complement(want) if rev else want), (i, R_, s, e)
            lifted += n
        assert [p[3] for p in mine] == sorted(p[3] for p in mine), i
        want_status = R.WHOLE if len(mine) == 1 and lifted == b - a else R.PARTIAL if lifted < b - a else R.SPLIT
        assert statuses[i] == want_status, i


def random_features(rng, source_length, n, invalid_p=0.1):
    out = []
    for _ in range(n):
        r = rng.randrange(len(source_length))
        L = source_length[r]
        a = rng.randrange(L)
        b = rng.choice((a + 1, L, rng.randint(a + 1, L)))
        if rng.random() < invalid_p:
            r, a, b = rng.choice(((len(source_length) + rng.randrange(3), a, b), (r, b, a), (r, a, a), (r, a, L + 1 + rng.randrange(5))))
        out.append((r, a, b))
    return out


def fuzz_case(seed, n_features=40):
    """-> (table, source_length, features).  Every third table is one round's table; the others are two rounds composed"""
    rng = random.Random(7000 + seed)
    base_len, inner, outer = CC.fuzz_case(seed, inner_pieces=(None, 1, 37)[seed % 3], outer_pieces=(4, 1, 12)[seed % 3])
    table = inner if seed % 3 == 1 else C.compose(outer, inner)
    return table, base_len, random_features(rng, base_len, n_features)


def sized_case(n_pieces, n_source, seed=0):
    """a table of n_pieces sequence pieces (and some gaps) over n_source source records of 64 bases, in records of up to five pieces;
    the pieces overlap and nest freely"""
    rng = random.Random(seed * 1000003 + n_pieces * 31 + n_source)
    source_length = [64] * n_source
    table, rec = [], []
    for j in range(n_pieces):
        r = rng.randrange(n_source) if j >= 2 else (0, n_source - 1)[j]   # (the first and the last source record are named)
        a = rng.randrange(64)
        rec.append((r, a, rng.randint(a + 1, 64), rng.choice((F, V))))
        if rng.random() < 0.2:
            rec.append((0, 0, rng.randint(1, 9), G))
        if len(rec) >= rng.randint(1, 5):
            table.append(rec)
            rec = []
    if rec:
        table.append(rec)
    return table, source_length


def sized_features(n, n_source, seed=0):
    rng = random.Random(seed * 7919 + n * 13 + n_source)
    out = []
    for i in range(n):
        r = (0, n_source - 1)[i] if i < 2 else rng.randrange(n_source + 1)   # (one past the last: INVALID)
        a = rng.randrange(64)
        out.append((r, a, rng.randint(a, 65)))   # (a == b and b == 65 are INVALID)
    return out


CARRY_CASES = [(1023, 4400), (1024, 4400), (262143, 262444), (262144, 262444)]   # (long_at, n_short)
CARRY_SECOND = 1000   # the second source record's short pieces


@functools.lru_cache(maxsize=None)
def carry_case(long_at, n_short):
    """-> (table, source_length, features, statuses): a table whose lookups live on the carries of the index's running maximum.
    Source record 0 is cut into n_short pieces [3 j, 3 j + 2) -- every third base is in no piece -- and ONE long piece from the gap
    base in front of 3 long_at to the record's end: it starts behind short piece long_at - 1 and in front of short piece long_at, so it
    takes place long_at of the sorted index, and whatever lies behind it there finds it only through rmax.  Behind it source record 1,
    cut the same way into CARRY_SECOND short pieces, with its long piece on the last place of a tile of the index: the running maximum
    starts over at the record's border, and behind that tile's border it is the carry again.  The pieces are dealt in shuffled order to
    table records of 1 to 40 pieces, so the table's order is not the index's"""
    rng = random.Random(9000 + long_at)
    assert 10 < long_at < n_short - 10
    n1 = CARRY_SECOND
    at1 = 1023 - (n_short + 1) % 1024   # (record 1's piece i has place n_short + 1 + i)
    assert 20 < at1 < n1 - 20
    source_length = [3 * n_short + 10, 3 * n1 + 10]
    pieces = []
    for r, n, at in ((0, n_short, long_at), (1, n1, at1)):
        pieces += [(r, 3 * j, 3 * j + 2, rng.choice((F, V))) for j in range(n)]
        pieces.append((r, 3 * at - 1, source_length[r], rng.choice((F, V))))
    rng.shuffle(pieces)
    table, at = [], 0
    while at < len(pieces):
        n = rng.randint(1, 40)
        table.append(pieces[at:at + n])
        at += n
    L0, L1 = source_length
    named = [
        ((0, L0 - 5, L0 - 1), R.WHOLE),                                     # in the long piece's far end, behind every short piece
        ((0, 3 * n_short - 1, 3 * n_short), R.WHOLE),                       # the last gap base: the long piece alone
        ((0, 3 * long_at + 5, 3 * long_at + 6), R.WHOLE),                   # a gap base just behind the long piece's place
        ((0, 3 * (long_at + 5), 3 * (long_at + 5) + 3), R.SPLIT),           # a short piece and its gap base there: both pieces
        ((0, 3 * (long_at - 10), 3 * (long_at - 10) + 2), R.WHOLE),         # in front of it: the short piece alone
        ((0, 3 * (long_at - 10) + 2, 3 * (long_at - 10) + 3), R.LOST),      # a gap base in front of it
        ((1, L1 - 5, L1 - 1), R.WHOLE),                                     # the second record: in its long piece's far end,
        ((1, 3 * (n1 - 1) + 2, 3 * n1), R.WHOLE),                           # on its last gap base,
        ((1, 15, 17), R.WHOLE),                                             # in front of its long piece
        ((1, 17, 18), R.LOST),                                              # and on a gap base there
    ]
    return table, source_length, [f for f, _ in named], [s for _, s in named]


@functools.lru_cache(maxsize=None)
def carry_expected(long_at, n_short):
    "the restatement's answer for carry_case's features, worked out once for all tests of a process (nobody changes it)"
    table, source_length, features, _ = carry_case(long_at, n_short)
    return R.lift(table, source_length, features)


def index_words(table):
    """the sorted index of a table as lift.h states it, in numpy: -> (key, word, start, end) with key[i] = (record << 32) | start in
    stable order and word[i] = (record << 32) | end, the words whose running maximum is rmax"""
    import numpy as np
    rows = np.array([p for rec in table for p in rec if p[3] != G], dtype=np.uint64).reshape(-1, 4)
    key = rows[:, 0] << np.uint64(32) | rows[:, 1]
    order = np.argsort(key, kind="stable")
    return key[order], (rows[:, 0] << np.uint64(32) | rows[:, 2])[order], rows[order, 1].astype(np.int64), rows[order, 2].astype(np.int64)


def table_text(table, source_length):
    "the head of a lift_check input file"
    words = [len(source_length)] + list(source_length) + [len(table)]
    for rec in table:
        words.append(len(rec))
        for p in rec:
            words.extend(p)
    return " ".join(map(str, words))
