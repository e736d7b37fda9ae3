"""Inputs of the assessment tests (tests/test_assess_cpu.py, tests/test_gpu_assess.py).  Plain Python: no GPU, no library.

BLOCK CASES are lists of kept blocks typed in directly (tuples in _synteny_restatement.FIELDS order), with the chains, breakpoints
and sums derived by hand in the comments: they pin the restatement and feed tools/assess_check.  ANCHOR CASES are anchor lists in
the manner of tests/_synteny_cases.py from which mxg_synteny_blocks makes such blocks, for the device: a block spec
(qrec, qpos, srec, spos, reverse, n) stands for n anchors 50 apart on either assembly, and the blocks call runs with max_gap = 100,
so that two specs never share a block as long as their nearest anchors lie more than 100 apart on one assembly."""
import random

from tests import _synteny_cases as cases

K = 32
STEP = 50
FWD, REV, GAP = 0, 1, 2


def blk(q_rec, q_start, s_rec, s_start, reverse=0, n=2):
    "the kept block a spec gives: n anchors STEP apart"
    span = STEP * (n - 1) + K
    return (n, q_rec, q_start, q_start + span, s_rec, s_start, s_start + span, reverse)


def block_case(blocks, q_len, s_len, pieces=None, first=None, k=K, **params):
    return dict(blocks=blocks, k=k, q_len=q_len, s_len=s_len, pieces=pieces, first=first, params=params)


def block_cases():
    """name -> (case, expected subset of the result).  A block of 2 anchors spans 82 bases: blk(.., 100, .., 1000) is q [100, 182),
    s [1000, 1082)"""
    out = {}
    # two blocks that a stray anchor split: same records, same direction, gq = 300 - 182 = 118 = gs: one chain of 2 blocks, 4 anchors
    out["stray_split"] = (block_case([blk(0, 100, 0, 1000), blk(0, 300, 0, 1200)], [1000], [5000]),
                          dict(n_chains=1, n_breakpoints=0, aligned_query=282, chained_subject=282, covered_subject=282,
                               chains=dict(n_blocks=[2], first_block=[0], n_anchors=[4], q_start=[100], q_end=[382], s_start=[1000], s_end=[1282])))
    # gq exactly 1 - k = -31: the next block starts at 182 - 31 = 151 (gs = 118): joined.  One base less, 150: not joined -- a relocation
    out["gq_least"] = (block_case([blk(0, 100, 0, 1000), blk(0, 151, 0, 1200)], [1000], [5000]), dict(n_chains=1))
    out["gq_below"] = (block_case([blk(0, 100, 0, 1000), blk(0, 150, 0, 1200)], [1000], [5000]),
                       dict(n_chains=2, breakpoints={(2, 0): 1}, bps=dict(chain=[0], kind=[2], at_join=[0], q_lo=[182], q_hi=[150])))
    # the same on the subject, forward (s_start 1082 - 31 = 1051) and reverse (the next block lies BELOW: its s_end = 1000 + 31 = 1031,
    # so s_start = 949; one more, 950, is one base too far in)
    out["gs_least"] = (block_case([blk(0, 100, 0, 1000), blk(0, 300, 0, 1051)], [1000], [5000]), dict(n_chains=1))
    out["gs_below"] = (block_case([blk(0, 100, 0, 1000), blk(0, 300, 0, 1050)], [1000], [5000]), dict(n_chains=2))
    out["gs_least_reverse"] = (block_case([blk(0, 100, 0, 1000, 1), blk(0, 300, 0, 949, 1)], [1000], [5000]),
                               dict(n_chains=1, chains=dict(s_start=[949], s_end=[1082], reverse=[1])))
    out["gs_below_reverse"] = (block_case([blk(0, 100, 0, 1000, 1), blk(0, 300, 0, 950, 1)], [1000], [5000]), dict(n_chains=2))
    # merge_gap 500 exactly on the query (gq = 682 - 182 = 500, gs = 118 with max_indel off), one more (683); the same on the subject
    out["merge_gap_q"] = (block_case([blk(0, 100, 0, 1000), blk(0, 682, 0, 1200)], [2000], [5000], merge_gap=500, max_indel=0), dict(n_chains=1))
    out["merge_gap_q_over"] = (block_case([blk(0, 100, 0, 1000), blk(0, 683, 0, 1200)], [2000], [5000], merge_gap=500, max_indel=0), dict(n_chains=2))
    out["merge_gap_s"] = (block_case([blk(0, 100, 0, 1000), blk(0, 300, 0, 1582)], [2000], [5000], merge_gap=500, max_indel=0), dict(n_chains=1))
    out["merge_gap_s_over"] = (block_case([blk(0, 100, 0, 1000), blk(0, 300, 0, 1583)], [2000], [5000], merge_gap=500, max_indel=0), dict(n_chains=2))
    # max_indel 1000: gq = 118, gs = 1118 (s_start 2200): |gq - gs| = 1000 joined; 2201: 1001, a relocation by distance
    out["max_indel"] = (block_case([blk(0, 100, 0, 1000), blk(0, 300, 0, 2200)], [1000], [5000]), dict(n_chains=1))
    out["max_indel_over"] = (block_case([blk(0, 100, 0, 1000), blk(0, 300, 0, 2201)], [1000], [5000]),
                             dict(n_chains=2, breakpoints={(2, 0): 1}))
    # that pair (indel 1001) in a record of three pieces, [0, 200) a GAP of 50 [250, 1000): base 181 lies in piece 0, base 300 in piece 2:
    # at a join, where join_indel = 100000 applies: joined.  In one piece of 1000 bases: not joined.  join_indel 1000: not joined, and
    # the breakpoint is blamed on the join
    three = [(0, 0, 200, FWD), (0, 0, 50, GAP), (0, 200, 950, FWD)]
    out["join_indel"] = (block_case([blk(0, 100, 0, 1000), blk(0, 300, 0, 2201)], [1000], [5000], three, [0, 3]), dict(n_chains=1))
    out["one_piece"] = (block_case([blk(0, 100, 0, 1000), blk(0, 300, 0, 2201)], [1000], [5000], [(0, 0, 1000, FWD)], [0, 1]), dict(n_chains=2))
    out["join_indel_over"] = (block_case([blk(0, 100, 0, 1000), blk(0, 300, 0, 2201)], [1000], [5000], three, [0, 3], join_indel=1000),
                              dict(n_chains=2, breakpoints={(2, 1): 1}, bps=dict(at_join=[1])))
    # the border inside the GAP piece itself: q_end - 1 = 181 in piece 0, q_start = 210 in the GAP piece 1: pieces differ, a join
    out["into_gap_piece"] = (block_case([blk(0, 100, 0, 1000), blk(0, 210, 0, 2201)], [1000], [5000], three, [0, 3]), dict(n_chains=1))
    # a turning anchor at q 150: forward [100, 182), then reverse [150, 232): an inversion with q_lo = 182 > q_hi = 150
    out["turning_anchor"] = (block_case([blk(0, 100, 0, 1000), blk(0, 150, 0, 968, 1)], [1000], [5000]),
                             dict(n_chains=2, breakpoints={(1, 0): 1}, bps=dict(chain=[0], kind=[1], at_join=[0], q_lo=[182], q_hi=[150])))
    # a translocation wins over a change of direction
    out["translocation"] = (block_case([blk(0, 100, 0, 1000), blk(0, 300, 1, 1200, 1)], [1000], [5000, 5000]),
                            dict(n_chains=2, breakpoints={(0, 0): 1}, bps=dict(kind=[0])))
    # a relocation by order: the next block lies behind on the subject (gs = 500 - 1082 < 1 - k)
    out["relocation_order"] = (block_case([blk(0, 100, 0, 1000), blk(0, 300, 0, 500)], [1000], [5000]),
                               dict(n_chains=2, breakpoints={(2, 0): 1}))
    # a record border between chains is no breakpoint
    out["record_border"] = (block_case([blk(0, 100, 0, 1000), blk(1, 100, 0, 3000)], [1000, 1000], [5000]),
                            dict(n_chains=2, n_breakpoints=0, bps=dict(chain=[])))
    # union over two subject records.  The chains, in query order:
    #   s0 [900, 1182) (6 anchors), s0 [1001, 1083) nested, s0 [1182, 1264)
    #   touching, s0 [3000, 3082) disjoint; s1 [1000, 1082) and s1 [1040, 1122) overlapping by 42.
    # record 0: 282 + 0 + 82 + 82 = 446; record 1: 82 + 40 = 122; covered 568; chained = 282 + 82 + 82 + 82 + 82 + 82 = 692
    out["union"] = (block_case([blk(0, 0, 0, 900, 0, 6), blk(1, 0, 0, 1001), blk(2, 0, 0, 1182), blk(3, 0, 0, 3000), blk(4, 0, 1, 1000), blk(5, 0, 1, 1040)],
                               [400] * 6, [5000, 5000]),
                    dict(n_chains=6, n_breakpoints=0, chained_subject=692, covered_subject=568, aligned_query=692))
    # Nx.  Chain spans 282 (6 anchors), 132 (3), 82, 82; S = 282, 414, 496, 578.
    #   na: D = query_bases = 564: 100 * 282 == 50 * 564 exactly -> N50 282 L50 1; 75 %: 423 > 414 -> j = 3: N75 82 L75 3; 90 %: 507.6 -> j = 4
    #   nga: D = subject_bases = 700: 50 %: 350 -> j = 2 (132); 75 %: 525 -> j = 4 (82); 90 %: 630 > 578: unreachable -> 0 0
    #   ng: query records 300, 164, 50, 50 against 700: S = 300, 464, 514, 564: 50 %: 350 -> j = 2 (164); 75 %: 525 -> j = 4 (50); 90 %: none
    out["nx"] = (block_case([blk(0, 0, 0, 0, 0, 6), blk(1, 0, 0, 1000, 0, 3), blk(2, 0, 0, 2000), blk(3, 0, 0, 3000)], [300, 164, 50, 50], [700]),
                 dict(n_chains=4, aligned_query=578, query_bases=564, subject_bases=700,
                      na=dict(n50=282, l50=1, n75=82, l75=3, n90=82, l90=4), nga=dict(n50=132, l50=2, n75=82, l75=4, n90=0, l90=0),
                      ng=dict(n50=164, l50=2, n75=50, l75=4, n90=0, l90=0)))
    # D == 0 on the subject side: nga and ng are zeros, na is not
    out["nx_d_zero"] = (block_case([blk(0, 0, 0, 0)], [100], [0]),
                        dict(nga=dict(n50=0, l50=0, n75=0, l75=0, n90=0, l90=0), ng=dict(n50=0, l50=0, n75=0, l75=0, n90=0, l90=0),
                             na=dict(n50=82, l50=1, n75=82, l75=1, n90=0, l90=0)))
    # zero blocks: zero chains, breakpoints and sums; ng still computed (400 of 600 reaches 50 %, 500 reaches 75 % = 450, not 90 % = 540)
    out["zero_blocks"] = (block_case([], [400, 100], [600]),
                          dict(n_blocks=0, n_chains=0, n_breakpoints=0, aligned_query=0, chained_subject=0, covered_subject=0,
                               breakpoints={(kind, j): 0 for kind in range(3) for j in range(2)},
                               na=dict(n50=0, l50=0, n75=0, l75=0, n90=0, l90=0), nga=dict(n50=0, l50=0, n75=0, l75=0, n90=0, l90=0),
                               ng=dict(n50=400, l50=1, n75=100, l75=2, n90=0, l90=0)))
    return out


def matches(got, expect):
    "does a result hold everything the expected subset names"
    for key, want in expect.items():
        have = got[key]
        if isinstance(want, dict):
            for sub, val in want.items():
                if [int(x) for x in have[sub]] != list(val) if isinstance(val, list) else int(have[sub]) != val:
                    return False
        elif int(have) != want:
            return False
    return True


def fuzz_block_case(i):
    "case i of the seeded sequence of block lists: a few query and subject records, stretches that chain, jumps, turns, tables"
    rng = random.Random(7000 + i)
    k = rng.choice([15, 32, 64])
    n_q, n_s = rng.choice([1, 2, 5]), rng.choice([1, 2, 3])
    blocks, q_rec, q_at, s_rec, s_at, rev = [], 0, 0, 0, 50000, 0
    for _ in range(rng.choice([0, 1, 2, 5, 30, 120])):
        n = rng.choice([2, 2, 3, 9])
        span_q, span_s = rng.randrange(k, 900) + k, rng.randrange(k, 900) + k
        roll = rng.random()
        if roll < 0.08 and q_rec + 1 < n_q:
            q_rec, q_at = q_rec + 1, 0
        elif roll < 0.16:
            s_rec = rng.randrange(n_s)
        elif roll < 0.26:
            rev ^= 1
        elif roll < 0.36:
            s_at = max(2000, s_at + rng.choice([-1, 1]) * rng.choice([1500, 40000]))
        q_start = max(0, q_at + rng.choice([1 - k, -k, -3, 0, 10, 400, 1000, 1001, 5000]))
        gs = rng.choice([1 - k, -k, 0, 10, 400, 999, 1400, 5000])
        s_start = max(0, s_at - gs - span_s) if rev else max(0, s_at + gs)
        blocks.append((n, q_rec, q_start, q_start + span_q, s_rec, s_start, s_start + span_s, rev))
        q_at, s_at = q_start + span_q, (s_start if rev else s_start + span_s)
    q_len = [max([b[3] for b in blocks if b[1] == r] + [0]) + rng.randrange(1, 300) for r in range(n_q)]
    s_len = [max([b[6] for b in blocks if b[4] == r] + [0]) + rng.randrange(0, 300) for r in range(n_s)]
    pieces = first = None
    if i % 2:
        pieces, first = [], [0]
        for r, ln in enumerate(q_len):
            at = sorted({0, ln} | {rng.randrange(1, ln) for _ in range(rng.choice([0, 1, 3, 12]))} if ln > 1 else {0, ln})
            for j, (lo, hi) in enumerate(zip(at, at[1:])):
                pieces.append((0, 0, hi - lo, GAP) if j % 3 == 1 else (r, lo, hi, rng.choice([FWD, REV])))
            first.append(len(pieces))
    return block_case(blocks, q_len, s_len, pieces, first, k=k, merge_gap=rng.choice([0, 1000, 100000]), max_indel=rng.choice([0, 10, 1000]),
                      join_indel=rng.choice([0, 1000, 100000]))


FUZZ_CASES = 100


# ---- anchor cases: what the device makes its blocks of --------------------------------------------------------------------------------
def spec_anchors(specs):
    "(qrec, qpos, srec, spos, reverse, n) -> anchors (qrec, qpos, srec, spos), n per spec, STEP apart, a reverse spec's subject falling"
    out = []
    for q_rec, q_pos, s_rec, s_pos, rev, n in specs:
        for i in range(n):
            out.append((q_rec, q_pos + STEP * i, s_rec, s_pos + STEP * ((n - 1 - i) if rev else i)))
    return out


def spec_case(specs, assess=None, **kw):
    "a synteny case (tests/_synteny_cases.py) whose blocks call gives one block per spec, and the assess parameters"
    kw.setdefault("max_gap", 100)
    case = cases.from_anchors(spec_anchors(specs), **kw)
    case["assess"] = dict(assess or {})
    case["n_specs"] = len(specs)
    return case


def anchor_cases():
    """name -> (case, expected subset), the block cases above that anchors can spell.  Left out are only the `_below` halves of the
    gq / gs pairs: a gap of exactly -k puts the next block's first anchor on this block's last one, and where two anchors share a
    place (and rise or fall together) that is the turning anchor -- see turning_anchor.  The zero-blocks and D == 0 cases are in
    tests/test_gpu_assess.py itself"""
    out = {}
    two = lambda q2, s2, **kw: spec_case([(0, 100, 0, 1000, 0, 2), (0, q2, 0, s2, 0, 2)], **kw)  # noqa: E731
    # gq exactly 1 - k: the second run starts one base past the first one's last anchor (150) and lies far off on the subject, which
    # is what ends the block there (max_gap 100); both bounds off, so only the `>= 1 - k` tests decide: q [100, 182), [151, 233)
    free = dict(merge_gap=0, max_indel=0)
    out["gq_least"] = (two(151, 5000, assess=free), dict(n_chains=1, chains=dict(q_start=[100], q_end=[233], s_start=[1000], s_end=[5082])))
    # gs exactly 1 - k, forward: s [1000, 1082), then [1051, 1133), far off on the query
    out["gs_least"] = (two(5000, 1051, assess=free), dict(n_chains=1, chains=dict(s_start=[1000], s_end=[1133])))
    # ... and reverse: the subject falls 1050, 1000, then 999, 949: s [1000, 1082), then [949, 1031): gs = 1000 - 1031
    out["gs_least_reverse"] = (spec_case([(0, 100, 0, 1000, 1, 2), (0, 5000, 0, 949, 1, 2)], assess=free),
                               dict(n_chains=1, chains=dict(s_start=[949], s_end=[1082], reverse=[1])))
    # a stray anchor on another subject record between two collinear runs: q 100, 150 | 200 (stray) | 300, 350
    out["stray_split"] = (cases.from_anchors([(0, 100, 0, 1000), (0, 150, 0, 1050), (0, 200, 1, 7000), (0, 300, 0, 1200), (0, 350, 0, 1250)], max_gap=0),
                          dict(n_blocks=2, n_chains=1, aligned_query=282, covered_subject=282, chains=dict(n_blocks=[2], n_anchors=[4])))
    out["stray_split"][0].update(assess={}, n_specs=2)
    out["merge_gap_q"] = (two(682, 1200, assess=dict(merge_gap=500, max_indel=0)), dict(n_chains=1))
    out["merge_gap_q_over"] = (two(683, 1200, assess=dict(merge_gap=500, max_indel=0)), dict(n_chains=2))
    out["merge_gap_s"] = (two(300, 1582, assess=dict(merge_gap=500, max_indel=0)), dict(n_chains=1))
    out["merge_gap_s_over"] = (two(300, 1583, assess=dict(merge_gap=500, max_indel=0)), dict(n_chains=2))
    out["max_indel"] = (two(300, 2200), dict(n_chains=1))
    out["max_indel_over"] = (two(300, 2201), dict(n_chains=2, breakpoints={(2, 0): 1}))
    # (the query record is 482 bases long here; through the table the second run moves from 300 to 350, so gq = 168 and gs = 1169)
    three = [(0, 0, 200, FWD), (0, 0, 50, GAP), (0, 200, 482, FWD)]
    out["join_indel"] = (two(300, 2251, pieces=three, first=[0, 3]), dict(n_chains=1))
    out["one_piece"] = (two(300, 2201, pieces=[(0, 0, 482, FWD)], first=[0, 1]), dict(n_chains=2, breakpoints={(2, 0): 1}))
    out["join_indel_over"] = (two(300, 2251, pieces=three, first=[0, 3], assess=dict(join_indel=1000)), dict(n_chains=2, breakpoints={(2, 1): 1}))
    # forward 100, 150, then the subject falls from the anchor at 150: it is in both blocks
    out["turning_anchor"] = (cases.from_anchors([(0, 100, 0, 1000), (0, 150, 0, 1050), (0, 200, 0, 1000 - 1)], max_gap=0),
                             dict(n_blocks=2, n_chains=2, breakpoints={(1, 0): 1}, bps=dict(q_lo=[182], q_hi=[150])))
    out["turning_anchor"][0].update(assess={}, n_specs=2)
    out["translocation"] = (spec_case([(0, 100, 0, 1000, 0, 2), (0, 300, 1, 1200, 1, 2)]), dict(n_chains=2, breakpoints={(0, 0): 1}))
    out["relocation_order"] = (two(300, 500), dict(n_chains=2, breakpoints={(2, 0): 1}))
    out["record_border"] = (spec_case([(0, 100, 0, 1000, 0, 2), (1, 100, 0, 3000, 0, 2)]), dict(n_chains=2, n_breakpoints=0))
    out["union"] = (spec_case([(0, 0, 0, 900, 0, 6), (1, 0, 0, 1001, 0, 2), (2, 0, 0, 1182, 0, 2), (3, 0, 0, 3000, 0, 2), (4, 0, 1, 1000, 0, 2),
                               (5, 0, 1, 1040, 0, 2)]), dict(n_chains=6, chained_subject=692, covered_subject=568))
    # spans 282, 132, 82, 82 (S = 282, 414, 496, 578) inside records of 300, 164, 100, 100 (664) against a subject of 828 bases:
    #   nga: 100 * 414 == 50 * 828 exactly -> N50 132 L50 2; 75 %: 621 > 578: unreachable.   na: 332 -> j = 2; 498 -> j = 4; 597.6: none
    #   ng: S = 300, 464, 564, 664: 414 -> j = 2 (164); 621 -> j = 4 (100); 745.2: none
    out["nx"] = (spec_case([(0, 0, 0, 0, 0, 6), (1, 0, 0, 300, 0, 3), (2, 0, 0, 450, 0, 2), (3, 0, 0, 550, 0, 2)], lengths=[[828], [300, 164, 100, 100]]),
                 dict(n_chains=4, query_bases=664, subject_bases=828,
                      na=dict(n50=132, l50=2, n75=82, l75=4, n90=0, l90=0), nga=dict(n50=132, l50=2, n75=0, l75=0, n90=0, l90=0),
                      ng=dict(n50=164, l50=2, n75=100, l75=4, n90=0, l90=0)))
    return out


def row_case(n, mode="chain", seed=0):
    """n blocks of two anchors on one query record, 200 apart.  chain: collinear, one chain.  apart: the subject rises by 2000 a block
    (indel 1800 > 1000), n chains in subject order.  reversed: the subject falls by 2000 a block, n chains in reverse subject order.
    interleaved: as apart, on two subject records in turn.  mixed: a seeded mix of all of these over three query records, 300 apart (a
    block may hold three anchors), with reverse blocks and joins"""
    rng = random.Random(seed)
    specs, seen, s_at = [], set(), 10 ** 6 if mode != "reversed" else 2000 * (n + 2)
    for b in range(n):
        if mode == "chain":
            specs.append((0, 200 * b, 0, 1000 + 200 * b, 0, 2))
        elif mode == "apart":
            specs.append((0, 200 * b, 0, 1000 + 2000 * b, 0, 2))
        elif mode == "reversed":
            specs.append((0, 200 * b, 0, s_at - 2000 * b, 0, 2))
        elif mode == "interleaved":
            specs.append((0, 200 * b, b % 2, 1000 + 2000 * (b // 2), 0, 2))
        else:
            roll = rng.random()
            s_at += 300 if roll < 0.6 else rng.choice([-5000, 1400, 5000, 150000])
            s_at = max(1000, s_at)
            while any(s_at + STEP * i in seen for i in range(3)):   # (no two minimizers in one place)
                s_at += 1
            seen.update(s_at + STEP * i for i in range(3))
            specs.append((b * 3 // max(n, 1), 300 * b, 0 if roll < 0.9 else 1, s_at, rng.choice([0, 0, 0, 1]), rng.choice([2, 2, 3])))
    return spec_case(specs)


def cover_case(m):
    """one chain of 60 blocks over s [1000, 12882) on query record 0, then m <= 2900 single blocks inside it on record 1, from the far
    end inwards (odd places: the chain's anchors lie on even ones)"""
    specs = [(0, 200 * b, 0, 1000 + 200 * b, 0, 2) for b in range(60)]
    specs += [(1, 200 * j, 0, 12799 - 4 * j, 0, 2) for j in range(m)]
    return spec_case(specs)
