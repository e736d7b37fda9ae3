"""Inputs of the many-records tests (tests/test_many_records_cpu.py, tests/test_gpu_many_records.py): anchor cases in the manner of
tests/_assess_cases.py whose number of RECORDS, not of anchors or blocks, is the size that grows.  Plain Python: no GPU, no library.

COUNTS are the record counts on either side of every change of the pass count of the sort of assess.hip, whose key is
s_record << 32 | s_start over 32 + bits_of(n_subject_records) bits, eight bits a pass: up to 255 records five passes (the result
lies in buffer 1), 256 to 65 535 six (buffer 0, the input's own), from 65 536 seven (buffer 1).  Eight passes take 2^24 records,
which no test of a few seconds builds; nothing here or in the tests that read this file reaches them.

A spec (qrec, qpos, srec, spos, reverse, n) is one block of n anchors, as in tests/_assess_cases.py; the blocks call runs with
max_gap = 100."""
import functools
import random

from tests import _assess_cases as AC, _synteny_cases as cases

K = AC.K
FWD, REV, GAP = 0, 1, 2
COUNTS = (1, 2, 127, 128, 255, 256, 257, 65535, 65536, 65537)
QUERY_COUNTS = (255, 256, 257, 1023, 1024, 1025, 65536, 65537)
MARKS = (0, 255, 256, 65535, 65536)   # the records on either side of a digit of the key (and the last one, n_s - 1)


def subject_blocks(n_s):
    "the number of blocks of many_subject_case: every record once, two more on up to six of them, and seeded ones behind"
    return 700 if n_s <= 257 else n_s + 164


def subject_specs(n_s, n_blocks, seed):
    "the specs of many_subject_case and the subject record of every block"
    rng = random.Random(seed)
    order = list(range(n_s))
    rng.shuffle(order)
    more = 2 * sorted({r for r in MARKS + (n_s - 1,) if r < n_s})
    rng.shuffle(more)
    order += more
    while len(order) < n_blocks:
        order.append(rng.randrange(n_s))
    order = order[:n_blocks]
    seen, specs = {}, []
    for b, r in enumerate(order):
        j = seen.get(r, 0)
        seen[r] = j + 1
        specs.append((0, 200 * b, r, 1000 + 40 * j, 1 if b % 5 == 4 else 0, 2))
    return specs, order


def many_subject_case(n_s, n_blocks=None, seed=0):
    """One query record with a block of two anchors (82 bases) every 200 bases; block b lies on subject record order[b]: a seeded
    shuffle of all n_s records, then two more blocks on each of the records 0, 255, 256, 65 535, 65 536 and n_s - 1 that exist
    (shuffled), then seeded records up to n_blocks.  The j-th block of a subject record starts at 1000 + 40 j, so that it overlaps
    the one before by 42 bases; every fifth block is reverse.  No two neighbours join (other records, or a subject gap of -42 < 1 - k):
    a chain per block, in an order on the subject that has nothing to do with the query's, in any digit.

    case["nx_lengths"]: lengths to hand to the blocks call instead of the true ones, for the Nx figures.  With the true ones (82 of
    every 200 query bases aligned, a subject of n_s records of more than 1000 bases) no Nx figure reaches 50 %, and the comparison
    would be 0 == 0.  The blocks call takes lengths as given where there is no table (tests/test_gpu_assess.py::
    test_subject_of_no_bases does the same): a query of 164 bases a block, which the chains reach to exactly 50 %, and subject
    records of 100 to 140 bases."""
    n_blocks = subject_blocks(n_s) if n_blocks is None else n_blocks
    specs, order = subject_specs(n_s, n_blocks, seed)
    case = AC.spec_case(specs)
    assert len(case["asms"][0]) == max(order) + 1
    case["order"] = order
    case["nx_lengths"] = [[100 + r % 41 for r in range(len(case["asms"][0]))], [164 * n_blocks]]
    return case


def with_two_record_subject(case):
    "the case with a third assembly (index 2) that holds every minimizer, a half on each of two records: a subject of two records on the same handle"
    n = sum(len(mxs) for _rid, mxs in case["asms"][1])
    half = n // 4 * 2   # (even: no block of two anchors lies across the border)
    two = [("low", [(cases._h(i), 7 * i) for i in range(half)]), ("high", [(cases._h(i), 7 * i) for i in range(half, n)])]
    return dict(case, asms=case["asms"] + [two], lengths=case["lengths"] + [[7 * n + K + 100] * 2])


def query_length(r):
    "the length of query record r of many_query_case: 47 values, 90 .. 136"
    return 90 + r * 37 % 47


def many_query_case(n_q):
    """Block b (two anchors, q [0, 82)) lies on query record b, on subject record b % 3 at 1000 + 100 (b // 3): n_q chains, no
    breakpoint, and record lengths of 47 values.  All lengths are the true ones: 82 of about 113 bases of every record are aligned,
    and the subject has about 100 bases a query record, so na, nga and ng all reach 50 %"""
    specs = [(b, 0, b % 3, 1000 + 100 * (b // 3), 1 if b % 5 == 4 else 0, 2) for b in range(n_q)]
    n_s = min(n_q, 3)
    lengths = [[1000 + 100 * ((n_q - 1 - r) // 3) + 82 + 18 for r in range(n_s)], [query_length(r) for r in range(n_q)]]
    return AC.spec_case(specs, lengths=lengths)


def few_chains_case(n_q):
    """n_q query records of which only 0, n_q // 2 and n_q - 1 hold minimizers: two collinear blocks each (gaps of 118 on either
    side), so six blocks and three chains, on three subject records; the other records are empty.  The lengths of the empty records
    take 97 values, and the subject's three records hold three quarters of the query's bases, so that ng counts thousands of
    records before it reaches 50 %"""
    specs = []
    for u, r in enumerate((0, n_q // 2, n_q - 1)):
        specs += [(r, 100, u, 1000, 0, 2), (r, 300, u, 1200, 0, 2)]
    case = AC.spec_case(specs)
    assert len(case["asms"][1]) == n_q
    carrying = {s[0] for s in specs}
    case["lengths"][1] = [ln if r in carrying else 40 + r * 31 % 97 for r, ln in enumerate(case["lengths"][1])]
    case["lengths"][0] = [max(ln, sum(case["lengths"][1]) // 4) for ln in case["lengths"][0]]
    return case


# ---- piece tables over the records of many_query_case ---------------------------------------------------------------------------------
def table_piece_per_record(case):
    "one piece per record, every other one REV, each its own table record"
    lengths = case["lengths"][case["q"]]
    return [(r, 0, ln, r % 2) for r, ln in enumerate(lengths)], list(range(len(lengths) + 1))


def table_dealt(case, seed=3):
    "the same pieces dealt into table records of 1 to 40 pieces, a GAP piece between two of them"
    rng = random.Random(seed)
    pool, _ = table_piece_per_record(case)
    pieces, first, at = [], [0], 0
    while at < len(pool):
        take = rng.randint(1, 40)
        for j, p in enumerate(pool[at:at + take]):
            if j:
                pieces.append((0, 0, rng.choice([1, 20, 100]), GAP))
            pieces.append(p)
        at += take
        first.append(len(pieces))
    return pieces, first


def table_high_falling(case, lowest=256):
    "pieces that name only the records at or above `lowest`, in falling record order, each its own table record"
    lengths = case["lengths"][case["q"]]
    pieces = [(r, 0, lengths[r], FWD) for r in range(len(lengths) - 1, lowest - 1, -1)]
    return pieces, list(range(len(pieces) + 1))


TABLES = {"piece_per_record": table_piece_per_record, "dealt": table_dealt, "high_falling": table_high_falling}


def names_for(n):
    "n names of 1 to 40 bytes"
    return ["q" * (13 * r % 40) + str(r % 10) for r in range(n)]


def paf_case(case):
    "the case through a table of one piece per record, so that the query's names are the caller's (tests/test_gpu_synteny.py::write_paf)"
    lengths = case["lengths"][case["q"]]
    out = dict(case, names=names_for(len(lengths)))
    out["pieces"], out["first"] = [(r, 0, ln, FWD) for r, ln in enumerate(lengths)], list(range(len(lengths) + 1))
    return out


# ---- the device's rule for the union, with a sort that reads only the low `bits` bits of the key ---------------------------------------
def cover_by_truncated_sort(chains, bits):
    """covered_subject as assess.hip computes it if its sort read `bits` key bits: a stable sort of the chains by
    (s_record << 32 | s_start) & mask, the running maximum of s_record << 32 | s_end in front of every chain, and as_uncovered of
    assess.h.  chains: (s_record, s_start, s_end)"""
    mask = (1 << bits) - 1
    run = total = 0
    for rec, lo, hi in sorted(chains, key=lambda c: (c[0] << 32 | c[1]) & mask):
        start = lo
        if run and run >> 32 == rec and (run & 0xFFFFFFFF) > start:
            start = run & 0xFFFFFFFF
        total += max(hi - start, 0)
        run = max(run, rec << 32 | hi)
    return total


@functools.lru_cache(maxsize=None)
def cached(builder, *args):
    "a case built once per process; the tests read it and leave it as it is"
    return globals()[builder](*args)


# ---- identity over short contigs: the two FASTA files ---------------------------------------------------------------------------------
TILE, SUB_TILE = 4096, 256   # the ingest's work tile and the sub-tile whose base counts text_of_base walks (ntjoin_amd/csrc/text_index.h)
N_RUN, LOWER, ONE_LINE, CRLF = 7, 11, 20, 30   # the contigs with an N run, in lower case, of one line, with "\r\n"


def fold(seq, width, eol="\n"):
    return "".join(seq[i:i + width] + eol for i in range(0, len(seq), width))


def short_contig_files(td, seed=29):
    """td/ref.fa: three records of about 50 kbp, 60 columns.  td/tgt.fa: 300 contigs of 200 to 900 bases cut from them in order (100 a
    record, a few bases skipped between two), 1 % substitutions, every third one reverse-complemented, 60 columns; contig N_RUN
    holds 25 N in its middle, contig LOWER is lower case, contig ONE_LINE stands on one line, contig CRLF ends its lines with
    "\\r\\n".  -> dict(ref, tgt: the paths; rtexts, ttexts: the sequence texts, line ends and all; contigs: the targets' bases)"""
    from tests import _identity_cases as IC
    rng = random.Random(seed)
    ref = [IC.rand_seq(rng, n) for n in (50000, 49000, 51000)]
    contigs = []
    for seq in ref:
        lens = [200, 900] + [rng.randint(200, 900) for _ in range(98)]
        rng.shuffle(lens)
        excess = sum(lens) - (len(seq) - 300)
        while excess > 0:
            i = rng.randrange(100)
            if 300 < lens[i] < 900:
                cut = min(excess, lens[i] - 201, 150)
                lens[i] -= cut
                excess -= cut
        skip, at = (len(seq) - sum(lens)) // 100, 0
        for n in lens:
            t = list(seq[at:at + n])
            for _ in range(n // 100):
                t[rng.randrange(n)] = rng.choice("ACGT")
            c = len(contigs)
            bases = "".join(t)
            if c % 3 == 1:
                bases = IC.revcomp(bases)
            if c == N_RUN:
                bases = bases[:n // 2] + "N" * 25 + bases[n // 2 + 25:]
            if c == LOWER:
                bases = bases.lower()
            contigs.append(bases)
            at += n + skip
    rtexts = [fold(seq, 60) for seq in ref]
    ttexts = [fold(seq, len(seq) if c == ONE_LINE else 60, "\r\n" if c == CRLF else "\n") for c, seq in enumerate(contigs)]
    out = dict(ref=str(td / "ref.fa"), tgt=str(td / "tgt.fa"), rtexts=rtexts, ttexts=ttexts, contigs=contigs)
    for path, ids, texts in ((out["ref"], [f"chr{r}" for r in range(3)], rtexts), (out["tgt"], [f"ctg{c}" for c in range(len(contigs))], ttexts)):
        with open(path, "w", newline="") as fh:
            for rid, text in zip(ids, texts):
                fh.write(f">{rid}\n{text}")
    return out


def tile_counts(data, tile):
    """of a FASTA file's bytes cut into tiles of `tile` bytes: (the tile borders that fall inside a record's sequence text, the tiles
    that hold sequence bytes of two records or more, the tiles)"""
    ranges, at = [], 0
    while at < len(data):
        assert data[at:at + 1] == b">"
        lo = data.index(b"\n", at) + 1
        at = data.find(b">", lo)
        at = len(data) if at < 0 else at
        ranges.append((lo, at))
    inside = sum(len(range((lo // tile + 1) * tile, hi, tile)) for lo, hi in ranges)
    held = {}
    for r, (lo, hi) in enumerate(ranges):
        for t in range(lo // tile, (hi - 1) // tile + 1):
            held.setdefault(t, set()).add(r)
    return inside, sum(1 for recs in held.values() if len(recs) >= 2), (len(data) + tile - 1) // tile
