"""Inputs of the synteny tests (tests/test_synteny_cpu.py, tests/test_gpu_synteny.py): hand-made cases with their expected blocks
typed in, shapes by size, and a seeded generator over a two-references-and-a-target universe in the manner of
tests/_format_cases.py: collinear stretches, reversed stretches, drop-outs, strays.  Plain Python: no GPU, no library.

An assembly is a list of (record id, [(hash, pos), ...]) with rising positions, as MxEngine.add_minimizers takes it once flattened.
A case is a dict: asms (references first, target last), lengths (one list per assembly), k, q, s, max_gap, min_anchors, min_span,
pieces / first (a piece table over the records of q, rows (record, start, end, kind), or None) and, for hand-made cases, expect
(the kept blocks as tuples in _synteny_restatement.FIELDS order), n_anchors_total and n_links."""
import random

K = 32
FWD, REV, GAP = 0, 1, 2


def _h(i):
    return 1_000_003 * (i + 1)


def from_anchors(anchors, extra_asm=False, **kw):
    """anchors: (qrec, qpos, srec, spos) -> a case of two assemblies, subject 0 and query 1, minimizer i being anchor i in both;
    extra_asm: a third assembly (index 2) that holds every minimizer too, in one record, so that all stay graph vertices"""
    def assembly(col):
        recs = {}
        for i, a in enumerate(anchors):
            recs.setdefault(a[col], []).append((_h(i), a[col + 1]))
        n = max(recs) + 1 if recs else 1
        return [(f"rec{r}", sorted(recs.get(r, []), key=lambda hp: hp[1])) for r in range(n)]
    asms = [assembly(2), assembly(0)]
    if extra_asm:
        asms.append([("all", [(_h(i), 7 * i) for i in range(len(anchors))])])
    case = dict(asms=asms, k=K, q=1, s=0, max_gap=0, min_anchors=2, min_span=0, pieces=None, first=None)
    case.update(kw)
    case.setdefault("lengths", [[max([p for _h_, p in mxs] + [0]) + K + 100 for _rid, mxs in asm] for asm in asms])
    return case


def graph_arrays(case):
    """what mxg_get_graph holds for the case: vertex_pos / vertex_record as [assembly][vertex], the vertices being the hashes that
    occur exactly once in every assembly (in the first assembly's order)"""
    where = []
    for asm in case["asms"]:
        seen = {}
        for r, (_rid, mxs) in enumerate(asm):
            for hsh, pos in mxs:
                seen.setdefault(hsh, []).append((r, pos))
        where.append(seen)
    verts = [hsh for _rid, mxs in case["asms"][0] for hsh, _pos in mxs if all(len(w.get(hsh, ())) == 1 for w in where)]
    vrec = [[w[hsh][0][0] for hsh in verts] for w in where]
    vpos = [[w[hsh][0][1] for hsh in verts] for w in where]
    return vpos, vrec


# ---- hand-made cases: the expected blocks are derived by hand in the comments ------------------------------------------------------
def hand_cases():
    out = {}
    # query positions 100 .. 500 of one record; the subject rises twice, then falls twice: + + - -.  The anchor at 300 is where the
    # direction turns and belongs to both blocks: anchors 100..300 -> q [100, 300 + 32), s [1000, 3000 + 32); anchors 300..500 ->
    # q [300, 532), s [min(3000, 2200), 3032), reverse
    out["turning_point"] = from_anchors(
        [(0, 100, 0, 1000), (0, 200, 0, 2000), (0, 300, 0, 3000), (0, 400, 0, 2500), (0, 500, 0, 2200)],
        expect=[(3, 0, 100, 332, 0, 1000, 3032, 0), (3, 0, 300, 532, 0, 2200, 3032, 1)], n_anchors_total=5, n_links=4)
    # max_gap 1000.  0 -> 1000: both distances exactly 1000, linked.  1000 -> 2001: 1001 on the query, not linked.  2001 -> 3001: 1000
    # and 1000, linked.  3001 -> 4000: 999 on the query but 4001 - 3000 = 1001 on the subject, not linked: the last anchor is alone
    out["max_gap_border"] = from_anchors(
        [(0, 0, 0, 0), (0, 1000, 0, 1000), (0, 2001, 0, 2000), (0, 3001, 0, 3000), (0, 4000, 0, 4001)], max_gap=1000,
        expect=[(2, 0, 0, 1032, 0, 0, 1032, 0), (2, 0, 2001, 3033, 0, 2000, 3032, 0)], n_anchors_total=5, n_links=2)
    # one REV piece [50, 400): anchors by falling position 300, 200, 100 -> 400 - (300 + 32) = 68, 400 - 232 = 168, 400 - 132 = 268;
    # the subject now falls 3000, 2000, 1000: one reverse block, q [68, 268 + 32), s [1000, 3032)
    out["rev_piece"] = from_anchors(
        [(0, 100, 0, 1000), (0, 200, 0, 2000), (0, 300, 0, 3000)], pieces=[(0, 50, 400, REV)], first=[0, 1],
        expect=[(3, 0, 68, 300, 0, 1000, 3032, 1)], n_anchors_total=3, n_links=2)
    # piece borders, k = 32, anchors at 100, 200, 300 and 1000.
    #   record 0 = FWD [100, 232): a == qpos takes 100 (-> 0), qpos + k == b takes 200 (-> 100); block q [0, 132), s [1000, 2032)
    #   record 1 = FWD [101, 332): a == qpos + 1 leaves 100 out; 200 -> 99, 300 + 32 == 332 -> 199; block q [99, 231), s [2000, 3032)
    #   record 2 = FWD [100, 231): 200 + 32 = 232 > b = 231 leaves 200 out; 100 alone makes no block
    # 100 and 200 lie in two pieces each and appear twice; 1000 lies in no piece and vanishes: 5 anchors, 2 links
    out["piece_borders"] = from_anchors(
        [(0, 100, 0, 1000), (0, 200, 0, 2000), (0, 300, 0, 3000), (0, 1000, 0, 9000)],
        pieces=[(0, 100, 232, FWD), (0, 101, 332, FWD), (0, 100, 231, FWD)], first=[0, 1, 2, 3],
        expect=[(2, 0, 0, 132, 0, 1000, 2032, 0), (2, 1, 99, 231, 0, 2000, 3032, 0)], n_anchors_total=5, n_links=2)
    # one record of three pieces: FWD [100, 232) (132 bases: 100 -> 0, 200 -> 100), a GAP of 10, REV [250, 400) at off = 142, which
    # takes 300 alone: 142 + (400 - 332) = 210.  0, 100, 210 over s 1000, 2000, 3000: one forward block q [0, 242)
    out["gap_and_offsets"] = from_anchors(
        [(0, 100, 0, 1000), (0, 200, 0, 2000), (0, 300, 0, 3000)], pieces=[(0, 100, 232, FWD), (0, 0, 10, GAP), (0, 250, 400, REV)],
        first=[0, 3], expect=[(3, 0, 0, 242, 0, 1000, 3032, 0)], n_anchors_total=3, n_links=2)
    # two query records and two subject records: a change of either record ends a block
    out["record_borders"] = from_anchors(
        [(0, 10, 0, 100), (0, 20, 0, 200), (0, 30, 1, 300), (0, 40, 1, 400), (1, 5, 1, 500), (1, 15, 1, 600), (1, 25, 1, 550)],
        expect=[(2, 0, 10, 52, 0, 100, 232, 0), (2, 0, 30, 72, 1, 300, 432, 0), (2, 1, 5, 47, 1, 500, 632, 0), (2, 1, 15, 57, 1, 550, 632, 1)],
        n_anchors_total=7, n_links=4)
    # min_anchors 3 drops the block of two; min_span 250 drops the first block of three (span 232) and keeps the second (span 432)
    out["filters"] = from_anchors(
        [(0, 0, 0, 0), (0, 100, 0, 100), (0, 200, 0, 200), (0, 300, 0, 150), (1, 0, 1, 0), (1, 200, 1, 200), (1, 400, 1, 400)],
        min_anchors=3, min_span=250, expect=[(3, 1, 0, 432, 1, 0, 432, 0)], n_anchors_total=7, n_links=5)
    return out


# ---- shapes by size ----------------------------------------------------------------------------------------------------------------
def line_case(n, reverse=False, **kw):
    "n anchors in one block (n >= 2), in either direction"
    return from_anchors([(0, 50 * i, 0, 70 * (n - 1 - i if reverse else i)) for i in range(n)], **kw)


def zigzag_case(n, **kw):
    "every inner anchor is a turning point: the subject goes up, down, up, ..."
    return from_anchors([(0, 50 * i, 0, 1000 + (i % 2) * 500 + i) for i in range(n)], **kw)


def nolink_case(n, **kw):
    "neighbours never share the subject record"
    return from_anchors([(0, 50 * i, i % 2, 70 * i) for i in range(n)], **kw)


def mixed_case(n, seed=1, **kw):
    "n anchors over a few records: stretches of random length and direction, a stray now and then"
    rng = random.Random(seed)
    anchors, seen, qrec, qpos, srec, spos, d = [], set(), 0, 0, 0, 10 ** 6, 1
    while len(anchors) < n:
        for _ in range(min(rng.choice([1, 2, 3, 7, 40, 300]), n - len(anchors))):
            qpos += rng.choice([40, 100, 900])
            spos += d * rng.choice([40, 100, 900])
            if spos < 1000:
                srec, spos = srec + 1, 10 ** 6
            while (srec, spos) in seen:
                spos += 1
            seen.add((srec, spos))
            anchors.append((qrec, qpos, srec, spos))
        roll = rng.random()
        if roll < 0.2:
            qrec, qpos = qrec + 1, 0
        elif roll < 0.4:
            srec, spos = srec + 1, 10 ** 6
        elif roll < 0.8:
            d = -d
        else:
            spos += rng.choice([-1, 1]) * 200_000
    return from_anchors(anchors, **kw)


def pieces_of(case, rng, many=None):
    """a random valid piece table over the records of the case's query: every record cut at random places (many: this many pieces
    for record 0), pieces reversed, dropped, doubled, gaps put between them, the pieces dealt to table records"""
    lengths = case["lengths"][case["q"]]
    pool = []
    for r, n in enumerate(lengths):
        cuts = many - 1 if many and r == 0 else rng.choice([0, 0, 1, 2, 5])
        at = sorted({0, n} | {rng.randrange(1, n) for _ in range(cuts)} if n > 1 else {0, n})
        for lo, hi in zip(at, at[1:]):
            if rng.random() < 0.12:
                continue
            pool.append((r, lo, hi, rng.choice([FWD, FWD, REV])))
            if rng.random() < 0.08:
                pool.append((r, max(0, lo - rng.randrange(40)), hi, rng.choice([FWD, REV])))
    if rng.random() < 0.3:
        rng.shuffle(pool)
    pieces, first = [], [0]
    while pool or len(first) == 1:
        take = len(pool) if many else rng.choice([1, 1, 2, 4])
        for j, p in enumerate(pool[:take]):
            if j and rng.random() < 0.3:
                pieces.append((0, 0, rng.choice([1, 20, 1000]), GAP))
            pieces.append(p)
        if not pool[:take]:
            pieces.append((0, 0, 5, GAP))
        pool = pool[take:]
        first.append(len(pieces))
    return pieces, first


def fuzz_case(i):
    "case i of the seeded sequence: three assemblies, the query and the subject among them, with or without a piece table"
    rng = random.Random(9000 + i)
    universe = [_h(j) for j in range(rng.choice([0, 1, 2, 3, 12, 60, 200, 500]))]
    asms = []
    for a in range(3):
        chunks, at = [], 0
        while at < len(universe):
            n = rng.choice([1, 2, 3, 5, 8, 20, 70])
            picks = [hsh for hsh in universe[at:at + n] if a == 2 or rng.random() < 0.93]   # drop-outs: no vertex
            at += n
            roll = rng.random()
            if a == 2 and roll < 0.3:
                picks.reverse()
            elif a == 2 and roll < 0.45 and len(picks) > 2:   # a stray
                u, v = rng.randrange(len(picks)), rng.randrange(len(picks))
                picks[u], picks[v] = picks[v], picks[u]
            if picks:
                chunks.append(picks)
        if a == 2:
            rng.shuffle(chunks)
        recs = []
        while chunks:
            take = rng.choice([1, 1, 2, 3])
            recs.append([hsh for c in chunks[:take] for hsh in c])
            chunks = chunks[take:]
        out = []
        for r, picks in enumerate(recs):
            pos, mxs = rng.randrange(200), []
            for hsh in picks:
                mxs.append((hsh, pos))
                pos += rng.choice([33, 100, 400, 999, 1001, 4000])
            out.append((f"a{a}r{r}", mxs))
        asms.append(out or [(f"a{a}r0", [])])
    lengths = [[max([p for _h_, p in mxs] + [0]) + K + rng.randrange(50) for _rid, mxs in asm] for asm in asms]
    q, s = rng.choice([(2, 0), (2, 1), (2, 0), (0, 2), (1, 0)])
    case = dict(asms=asms, lengths=lengths, k=K, q=q, s=s, max_gap=rng.choice([0, 999, 1000, 5000]), min_anchors=rng.choice([2, 3, 5]),
                min_span=rng.choice([0, 0, 500]), pieces=None, first=None)
    if i % 2:
        case["pieces"], case["first"] = pieces_of(case, rng)
    return case


FUZZ_CASES = 100
