"""GPU tests of mxg_identity_segments (include/ntjoin_mx.h, row f14) against the plain DP of tests/_identity_restatement.py: the hand
cases, the boundary shapes (lengths around the word, the band and the tile; every shift; blocks that reach and pass the band's edge;
saturation; max_seg; class 4 inside and just outside; lower case and U), each also reversed, seeded mutated pairs, text layouts
(lines of 60 columns and of one, "\\r\\n", tile borders, a record's last tile), segment counts around the wave, one text as both
sides, the kept scaffold text, and every refusal with the handle usable afterwards; then of mxg_synteny_identity and the PAF tags of
mxg_write_synteny_paf_ex against the restatement run over mxg_get_graph's arrays and the FASTA strings: a mutated, cut-up copy of a
reference directly and through the scaffolds' piece table, no block, one block, a block of 4097 anchors, foreign tables, small
windows.  The FASTA files are written here."""
import random

import numpy as np
import pytest

from tests import _identity_cases as cases, _identity_restatement as R

pytestmark = pytest.mark.gpu

EINVAL = -1


def fold(seq, width, eol="\n"):
    return "".join(seq[i:i + width] + eol for i in range(0, len(seq), width))


def write_fasta(path, records, widths, eols=None):
    "records: [(id, bases)]; record r is folded at widths[r] columns with line end eols[r] -> the sequence texts, line ends and all"
    texts = [fold(seq, widths[r], (eols or ["\n"] * len(records))[r]) for r, (_rid, seq) in enumerate(records)]
    with open(path, "w", newline="") as fh:
        for (rid, _seq), text in zip(records, texts):
            fh.write(f">{rid}\n{text}")
    return texts


class Layout:
    """Intervals laid out in the records of one file, one behind the other, with what stands between them chosen in turn from
    SEPS: nothing, one class-4 base (directly outside both neighbours), a few valid bases."""
    SEPS = ["", "N", "ac", "n", "GT-"]

    def __init__(self, n_records):
        self.seq = [""] * n_records
        self.n = 0

    def put(self, interval):
        r = self.n % len(self.seq)
        self.seq[r] += self.SEPS[self.n % len(self.SEPS)]
        self.n += 1
        at = len(self.seq[r])
        self.seq[r] += interval
        return r, at


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    """Every case of the hand list, the boundary shapes and 300 mutated pairs, laid out in a query file of three records (60 columns,
    1 column, 70 columns with "\\r\\n") and a subject file of two (61 columns, 80 with "\\r\\n"), and what the restatement says of
    them, computed once."""
    td = tmp_path_factory.mktemp("identity_shapes")
    all_cases = [c[:5] for c in cases.HAND] + cases.boundary_cases() + cases.mutated_pairs(300, seed=3)
    ql, sl = Layout(3), Layout(2)
    segs = []
    for _name, q, s, rev, _m in all_cases:
        (qr, qs), (sr, ss) = ql.put(q), sl.put(s)
        segs.append((qr, qs, len(q), sr, ss, len(s), rev))
    qtexts = write_fasta(td / "q.fa", [(f"q{r}", seq + "ACGT") for r, seq in enumerate(ql.seq)], [60, 1, 70], ["\n", "\n", "\r\n"])
    stexts = write_fasta(td / "s.fa", [(f"s{r}", seq + "N") for r, seq in enumerate(sl.seq)], [61, 80], ["\n", "\r\n"])
    want = [R.segment_of_records(qtexts, stexts, seg, c[4]) for seg, c in zip(segs, all_cases)]
    # (the layout changes nothing: the same answers as for the bare strings)
    assert want == [R.segment(q, s, bool(rev), m) for _n, q, s, rev, m in all_cases]
    return {"cases": all_cases, "segs": segs, "want": want, "q": str(td / "q.fa"), "s": str(td / "s.fa")}


def as_tuples(got):
    return list(zip(got["edits"].tolist(), got["status"].tolist(), got["saturated"].astype(int).tolist()))


def engine(**kw):
    from ntjoin_amd.engine import MxEngine
    return MxEngine(k=15, w=10, **kw)


def test_shapes_and_pairs(shapes):
    with engine() as eng:
        q, s = eng.add_fasta("q", 1.0, shapes["q"]), eng.add_fasta("s", 1.0, shapes["s"])
        by_max_seg = {}
        for i, c in enumerate(shapes["cases"]):
            by_max_seg.setdefault(c[4], []).append(i)
        seen = 0
        for max_seg, idx in sorted(by_max_seg.items()):
            got = as_tuples(eng.identity_segments(q, s, [shapes["segs"][i] for i in idx], max_seg=max_seg))
            for i, g in zip(idx, got):
                assert g == shapes["want"][i], (shapes["cases"][i][0], g, shapes["want"][i])
            seen += len(idx)
        assert seen == len(shapes["cases"])
    for c, w in zip(cases.HAND, shapes["want"]):  # (the hand cases come first)
        assert w == c[5], c[0]
    states = {(w[1], w[2]) for w in shapes["want"]}
    assert states == {(0, 0), (0, 1), (1, 0), (2, 0), (3, 0)}  # aligned, saturated and the three skips all occur


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    "two files of three records of about 10 kbp each, the second a mutated copy of the first; 60 columns, 1 column, 77 with \\r\\n"
    td = tmp_path_factory.mktemp("identity_genome")
    rng = random.Random(17)
    a = [cases.rand_seq(rng, n) for n in (10007, 9000, 12289)]
    b = []
    for seq in a:
        t = list(seq)
        for _ in range(len(t) // 100):
            t[rng.randrange(len(t))] = rng.choice("ACGT")
        b.append("".join(t))
    ta = write_fasta(td / "a.fa", [(f"a{r}", s) for r, s in enumerate(a)], [60, 1, 77], ["\n", "\n", "\r\n"])
    tb = write_fasta(td / "b.fa", [(f"b{r}", s) for r, s in enumerate(b)], [60, 80, 4096])
    return {"a": str(td / "a.fa"), "b": str(td / "b.fa"), "ta": ta, "tb": tb, "seq_a": a, "seq_b": b}


def check(eng, qa, sa, qtexts, stexts, segs, max_seg=10000):
    got = as_tuples(eng.identity_segments(qa, sa, segs, max_seg=max_seg))
    cache = {}
    for seg, g in zip(segs, got):
        key = tuple(seg)
        if key not in cache:
            cache[key] = R.segment_of_records(qtexts, stexts, seg, max_seg)
        assert g == cache[key], (seg, g, cache[key])
    return got


def test_text_layout(genome):
    """intervals chosen by where their bytes lie: from the last base of a line, across every 4096-byte border of the file, in a
    record's last tile up to its last base, in the record of one-base lines and in the one with "\\r\\n" """
    segs = []
    for r in range(3):
        n = len(genome["seq_a"][r])
        segs += [(r, 59, 200, r, 59, 200, 0), (r, 59, 1, r, 59, 1, 0), (r, 0, 61, r, 0, 60, 1), (r, n - 300, 300, r, n - 310, 310, 0),
                 (r, n - 1, 1, r, n - 1, 1, 1), (r, n - 4000, 4000, r, n - 4000, 4000, 1)]
    segs.append((0, 0, len(genome["seq_a"][0]) - 5, 0, 0, len(genome["seq_a"][0]) - 5, 0))
    # a file's byte c * 4096 lies in record 0 about base c * 4096 * 60 / 61 - 4: intervals of 200 bases that straddle it, and ones
    # that begin or end right at it
    for c in (1, 2):
        at = c * 4096 * 60 // 61 - 4
        for d in (-100, -8, -1, 0, 1, 8):
            segs.append((0, at + d - 50, 200, 0, at + d - 60, 215, 0))
            segs.append((0, at + d, 100, 0, at + d, 100, 1))
    with engine() as eng:
        a, b = eng.add_fasta("a", 1.0, genome["a"]), eng.add_fasta("b", 1.0, genome["b"])
        got = check(eng, a, b, genome["ta"], genome["tb"], segs, max_seg=20000)
        assert sum(1 for g in got if g[1] == R.ALIGNED and not g[2]) > 20
        got = check(eng, b, a, genome["tb"], genome["ta"], segs, max_seg=20000)
        assert any(g[1] == R.ALIGNED and g[0] > 0 for g in got)


def test_one_text_on_both_sides(genome):
    pal = "ACGTTGCATGCAACGT"
    assert cases.revcomp(pal) == pal
    with engine() as eng:
        a = eng.add_fasta("a", 1.0, genome["a"])
        segs = [(1, 500, 700, 1, 500, 700, 0), (1, 500, 700, 1, 500, 700, 1), (0, 10, 40, 2, 10, 40, 0), (2, 100, 300, 2, 110, 300, 0)]
        got = check(eng, a, a, genome["ta"], genome["ta"], segs)
        assert got[0] == (0, R.ALIGNED, 0) and got[1][2] == 1


def test_palindrome_in_a_file(tmp_path):
    pal = "ACGTTGCATGCAACGT" * 8
    assert cases.revcomp(pal) == pal
    texts = write_fasta(tmp_path / "p.fa", [("p", "GG" + pal + "TT"), ("r", "A")], [7, 60])
    with engine() as eng:
        a = eng.add_fasta("p", 1.0, str(tmp_path / "p.fa"))
        got = check(eng, a, a, texts, texts, [(0, 2, len(pal), 0, 2, len(pal), 1), (0, 2, len(pal), 0, 2, len(pal), 0), (1, 0, 1, 1, 0, 1, 1)])
        assert got == [(0, R.ALIGNED, 0), (0, R.ALIGNED, 0), (1, R.ALIGNED, 0)]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 65537])
def test_segment_counts(genome, n):
    rng = random.Random(n)
    longest = 8 if n > 1000 else 90
    segs = []
    for _ in range(n):
        r, lq, ls = rng.randrange(3), rng.randint(1, longest), rng.randint(1, longest)
        at = rng.randrange(len(genome["seq_a"][r]) - 200)
        segs.append((r, at, lq, r, at + rng.randint(0, 2), ls, rng.randrange(2) if n < 1000 else 0))
    with engine() as eng:
        a, b = eng.add_fasta("a", 1.0, genome["a"]), eng.add_fasta("b", 1.0, genome["b"])
        got = eng.identity_segments(a, b, segs)
        assert len(got["edits"]) == len(got["status"]) == len(got["saturated"]) == n
        if n <= 1000:
            check(eng, a, b, genome["ta"], genome["tb"], segs)
            return
        # past 2^16: the restatement once per distinct pair of class strings (a few thousand among 65 537 segments of 1 .. 8 bases)
        cache, qb, sb = {}, [R.bases(t) for t in genome["ta"]], [R.bases(t) for t in genome["tb"]]
        for seg, g in zip(segs, as_tuples(got)):
            key = (qb[seg[0]][seg[1]:seg[1] + seg[2]], sb[seg[3]][seg[4]:seg[4] + seg[5]])
            if key not in cache:
                cache[key] = R.segment(*key)
            assert g == cache[key], (seg, g)


def test_one_long_lane_in_a_wave(genome):
    segs = [(0, 5 + i, 1, 0, 5 + i, 1, 0) for i in range(64)]
    segs[37] = (2, 100, 4097, 2, 100, 4097, 0)
    with engine() as eng:
        a, b = eng.add_fasta("a", 1.0, genome["a"]), eng.add_fasta("b", 1.0, genome["b"])
        got = check(eng, a, b, genome["ta"], genome["tb"], segs)
        assert got[37][1] == R.ALIGNED and got[37][0] > 0 and all(g[0] <= 1 for i, g in enumerate(got) if i != 37)


def scaffold_run(eng, a, tmp_path, keep=True):
    "two paths over the records of assembly a, one with a REV node and a gap -> the records of the kept text, in its order"
    rows = [(0, 100, 2000, 5, 0, 0, 0), (1, 0, 1500, 0, 0, 0, 1), (2, 3000, 6000, 12, 0, 0, 1), (0, 4000, 9000, 0, 0, 0, 0)]
    fa, ufa = tmp_path / "assigned.fa", tmp_path / "unassigned.fa"
    eng.write_scaffolds(a, rows, [0, 2, 4], assigned=fa, unassigned=ufa, keep=keep)
    recs = []
    for path in (fa, ufa):
        for chunk in path.read_text().split(">")[1:]:
            recs.append(chunk.split("\n", 1)[1])
    return recs


def test_kept_scaffold_text(genome, tmp_path):
    with engine() as eng:
        a, b = eng.add_fasta("a", 1.0, genome["a"]), eng.add_fasta("b", 1.0, genome["b"])
        scaf = scaffold_run(eng, a, tmp_path)
        pieces, first, ids = eng.scaffold_pieces()
        assert len(scaf) == len(ids) >= 5 and [len(R.bases(t)) for t in scaf] == \
            [int(sum(int(p["end"]) - int(p["start"]) for p in pieces[first[r]:first[r + 1]])) for r in range(len(ids))]
        from ntjoin_amd import capi
        # scaffold 0 = a0[100, 2000) + 5 N + revcomp(a1[0, 1500)); scaffold 1 = revcomp(a2[3000, 6000)) + 12 N + a0[4000, 9000)
        segs = [(0, 0, 1900, 0, 100, 1900, 0), (0, 1905, 1500, 1, 0, 1500, 1), (0, 1890, 30, 0, 1990, 30, 0), (0, 1905, 2, 1, 1498, 2, 1),
                (1, 0, 3000, 2, 3000, 3000, 1), (1, 3012, 5000, 0, 4000, 5000, 0), (1, 3011, 20, 0, 4000, 19, 0)]
        for r in range(2, len(ids)):  # the unassigned records against where they were cut from, whole and their last base
            p = pieces[first[r]]
            n = int(p["end"]) - int(p["start"])
            segs += [(r, 0, min(n, 2000), int(p["record"]), int(p["start"]), min(n, 2000), 0), (r, n - 1, 1, int(p["record"]), int(p["end"]) - 1, 1, 0)]
        got = check(eng, capi.TEXT_SCAFFOLDS, a, scaf, genome["ta"], segs)
        assert got[0] == got[1] == got[4] == got[5] == (0, R.ALIGNED, 0) and got[2][1] == got[6][1] == R.SKIP_N and got[3][1] == R.ALIGNED
        assert all(g == (0, R.ALIGNED, 0) for g in got[7:])
        check(eng, capi.TEXT_SCAFFOLDS, b, scaf, genome["tb"], segs)                 # against the mutated copy
        check(eng, b, capi.TEXT_SCAFFOLDS, genome["tb"], scaf, [(s[3], s[4], s[5], s[0], s[1], s[2], s[6]) for s in segs])
        check(eng, capi.TEXT_SCAFFOLDS, capi.TEXT_SCAFFOLDS, scaf, scaf, [(0, 10, 500, 1, 3020, 510, 0), (1, 5, 100, 1, 5, 100, 1)])
        from ntjoin_amd.engine import MxError
        with pytest.raises(MxError) as err:   # beyond a kept record's end
            eng.identity_segments(capi.TEXT_SCAFFOLDS, a, [(0, 3400, 6, 0, 0, 6, 0)])
        assert err.value.code == EINVAL
        scaffold_run(eng, a, tmp_path, keep=False)   # the next call keeps nothing
        with pytest.raises(MxError) as err:
            eng.identity_segments(capi.TEXT_SCAFFOLDS, a, segs[:1])
        assert err.value.code == EINVAL and "kept no text" in str(err.value)


def test_refusals(genome, tmp_path):
    from ntjoin_amd import capi
    from ntjoin_amd.engine import MxError
    with engine() as eng:
        a, b = eng.add_fasta("a", 1.0, genome["a"]), eng.add_fasta("b", 1.0, genome["b"])
        eng.sketch(a)
        tsv = str(tmp_path / "a.tsv")
        eng.write_tsv(a, tsv)
        t = eng.add_tsv("from_tsv", 1.0, tsv)
        good = [(0, 10, 50, 0, 10, 50, 0)]
        n0 = len(genome["seq_a"][0])

        def refused(q, s, segs, match, **kw):
            with pytest.raises(MxError) as err:
                eng.identity_segments(q, s, segs, **kw)
            assert err.value.code == EINVAL and match in str(err.value), str(err.value)
            check(eng, a, b, genome["ta"], genome["tb"], good)  # (the handle goes on)

        refused(a, b, good + [(0, n0 - 10, 11, 0, 0, 11, 0)], "segment 1: query bases")
        refused(a, b, [(0, 0, 11, 0, n0 - 10, 11, 1)], "segment 0: subject bases")
        refused(a, b, [(0, 0xFFFFFFF0, 0x20, 0, 0, 5, 0)], "query bases")
        refused(a, b, good + [(0, 5, 0, 0, 5, 3, 0)], "lq = 0")
        refused(a, b, [(0, 5, 3, 0, 5, 0, 0)], "ls = 0")
        refused(a, b, [(3, 5, 3, 0, 5, 3, 0)], "no query record 3")
        refused(a, b, [(0, 5, 3, 3, 5, 3, 0)], "no subject record 3")
        refused(t, b, good, "does not hold")
        refused(a, t, good, "does not hold")
        refused(a, 7, good, "no assembly 7")
        refused(capi.TEXT_SCAFFOLDS, b, good, "kept no text")
        refused(a, b, good, "max_seg", max_seg=0)
        assert as_tuples(eng.identity_segments(a, b, [])) == []


# ---- mxg_synteny_identity: the segments of the kept blocks --------------------------------------------------------------------------
K, W = 15, 10
BLOCKS_KW = dict(max_gap=100000, min_anchors=3, min_span=0)


def parse_fasta(path):
    "-> (ids, sequence texts with their line ends)"
    ids, texts = [], []
    with open(path, newline="") as fh:
        for chunk in fh.read().split(">")[1:]:
            head, _, text = chunk.partition("\n")
            ids.append(head.split()[0])
            texts.append(text)
    return ids, texts


def piece_rows(pieces):
    return [(int(p["record"]), int(p["start"]), int(p["end"]), int(p["kind"])) for p in pieces]


def restated_identity(eng, q, s, qtexts, stexts, pieces=None, first=None, max_seg=10000, **kw):
    from tests import _synteny_restatement as SR
    g = eng.get_graph()
    anchors = SR.anchor_list(g["vertex_pos"], g["vertex_record"], q, s, K, None if pieces is None else piece_rows(pieces),
                             None if first is None else [int(x) for x in first])
    return R.synteny_identity(anchors, K, qtexts, stexts, max_seg=max_seg, **dict(BLOCKS_KW, **kw))


def same_identity(got, want):
    assert {n: got[n] for n in R.SUM_FIELDS} == {n: want[n] for n in R.SUM_FIELDS}
    for name in R.BLOCK_FIELDS:
        assert got["blocks"][name].tolist() == want["blocks"][name], name


def paf_with_tags(plain, got):
    lines = plain.decode().splitlines()
    assert len(lines) == got["n_blocks"]
    b = got["blocks"]
    return "".join(line + R.paf_tags(int(b["aligned_q"][i]), int(b["aligned_s"][i]), int(b["edits"][i])) + "\n" for i, line in enumerate(lines)).encode()


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """a reference of 3 records of about 40 kbp folded at 60, and a target made from it: cut into contigs, 1 % substitutions, an
    indel of 1 .. 40 bases about every 2 kbp, one N run, one contig reverse-complemented, some lower case"""
    td = tmp_path_factory.mktemp("identity_pair")
    rng = random.Random(23)
    ref = [cases.rand_seq(rng, n) for n in (40000, 39000, 41000)]
    contigs = []
    for r, seq in enumerate(ref):
        cuts = [0] + sorted(rng.sample(range(8000, len(seq) - 8000), 2)) + [len(seq)]
        for c in range(3):
            t = list(seq[cuts[c]:cuts[c + 1]])
            for _ in range(len(t) // 100):
                t[rng.randrange(len(t))] = rng.choice("ACGT")
            at = rng.randrange(500, 2500)
            while at < len(t) - 100:
                b = rng.randint(1, 40)
                if rng.random() < 0.5:
                    t[at:at] = list(cases.rand_seq(rng, b))
                else:
                    del t[at:at + b]
                at += rng.randrange(1000, 3000)
            contigs.append("".join(t))
    contigs[2] = contigs[2][:3000] + "N" * 40 + contigs[2][3040:]
    contigs[4] = cases.revcomp(contigs[4])
    contigs[5] = contigs[5][:2000] + contigs[5][2000:5000].lower() + contigs[5][5000:]
    rtexts = write_fasta(td / "ref.fa", [(f"chr{r}", s) for r, s in enumerate(ref)], [60] * 3)
    ttexts = write_fasta(td / "tgt.fa", [(f"ctg{c}", s) for c, s in enumerate(contigs)], [70] * len(contigs))
    return {"ref": str(td / "ref.fa"), "tgt": str(td / "tgt.fa"), "rtexts": rtexts, "ttexts": ttexts, "contigs": contigs}


def load_pair(pair):
    eng = engine()
    r, t = eng.add_fasta("ref", 2.0, pair["ref"]), eng.add_fasta("tgt", 1.0, pair["tgt"])
    eng.sketch()
    eng.build_graph()
    return eng, r, t


def test_blocks_direct_and_through_the_scaffolds_table(pair, tmp_path):
    eng, r, t = load_pair(pair)
    with eng:
        # the target as loaded
        blk = eng.synteny_blocks(t, r, **BLOCKS_KW)
        got = eng.synteny_identity()
        want = restated_identity(eng, t, r, pair["ttexts"], pair["rtexts"])
        same_identity(got, want)
        assert got["n_blocks"] == blk["n_blocks"] >= 9 and got["n_segments"] == int(blk["n_anchors"].sum()) > 5000
        assert got["n_skip_n"] >= 1 and got["n_skip_shift"] >= 1 and got["n_aligned"] > 5000 and any(blk["reverse"])
        assert got["block_q"] == int((blk["q_end"].astype(np.int64) - blk["q_start"]).sum())
        assert 0 < got["edits"] < got["aligned_q"] // 20   # (1 % substitutions and a few indels)
        # the blocks, their PAF and the assessment go on as before; the tags are those of the Python formatter
        again = eng.synteny_blocks(t, r, **BLOCKS_KW)
        assert all(again[n].tolist() == blk[n].tolist() for n in eng.SYNTENY_FIELDS)
        from ntjoin_amd.engine import MxError
        with pytest.raises(MxError) as err:   # no identity since that blocks call
            eng.write_synteny_paf(tmp_path / "no.paf", identity=True)
        assert err.value.code == EINVAL and "mxg_synteny_identity" in str(err.value)
        eng.write_synteny_paf(tmp_path / "plain.paf")
        same_identity(eng.synteny_identity(), want)
        chains = eng.synteny_assess()["n_chains"]
        eng.write_synteny_paf(tmp_path / "flags0.paf", identity=False)
        eng.write_synteny_paf(tmp_path / "tags.paf", identity=True)
        assert eng.synteny_assess()["n_chains"] == chains > 0
        plain = (tmp_path / "plain.paf").read_bytes()
        assert (tmp_path / "flags0.paf").read_bytes() == plain and plain.count(b"\n") == got["n_blocks"]
        assert (tmp_path / "tags.paf").read_bytes() == paf_with_tags(plain, got)
        # max_seg: segments of more than 20 bases on either side are counted
        small = eng.synteny_identity(max_seg=20)
        same_identity(small, restated_identity(eng, t, r, pair["ttexts"], pair["rtexts"], max_seg=20))
        assert small["n_skip_len"] > 0 and small["n_segments"] == got["n_segments"]
        # the scaffolds: two paths with a REV node and gaps, the rest unassigned
        n = [len(c) for c in pair["contigs"]]
        rows = [(0, 0, n[0], 7, 0, 0, 0), (1, 0, n[1], 100, 0, 0, 1), (2, 50, n[2] - 100, 0, 0, 0, 0), (5, 100, n[5], 1, 0, 0, 1), (3, 0, n[3] - 2000, 0, 0, 0, 0)]
        fa, ufa = tmp_path / "assigned.fa", tmp_path / "unassigned.fa"
        eng.write_scaffolds(t, rows, [0, 3, 5], assigned=fa, unassigned=ufa, keep=True)
        ids, scaf = parse_fasta(fa)
        ids2, scaf2 = parse_fasta(ufa)
        pieces, first, kept_ids = eng.scaffold_pieces()
        assert kept_ids == ids + ids2 and len(ids) == 2
        blk = eng.synteny_blocks(t, r, pieces=pieces, first=first, **BLOCKS_KW)
        got = eng.synteny_identity()
        same_identity(got, restated_identity(eng, t, r, scaf + scaf2, pair["rtexts"], pieces=pieces, first=first))
        assert got["n_blocks"] == blk["n_blocks"] >= 9 and got["n_aligned"] > 5000
        eng.write_synteny_paf(tmp_path / "scaf.paf", query_names=kept_ids)
        eng.write_synteny_paf(tmp_path / "scaf_tags.paf", query_names=kept_ids, identity=True)
        eng.write_synteny_paf(tmp_path / "scaf_tags.paf", query_names=kept_ids, identity=True, append=True)
        assert (tmp_path / "scaf_tags.paf").read_bytes() == 2 * paf_with_tags((tmp_path / "scaf.paf").read_bytes(), got)
        # a foreign table: one piece per contig is not what the kept text was written from
        eng.synteny_blocks(t, r, pieces=[(c, 0, n[c], 0) for c in range(len(n))], first=list(range(len(n) + 1)), **BLOCKS_KW)
        with pytest.raises(MxError) as err:
            eng.synteny_identity()
        assert err.value.code == EINVAL and "piece table" in str(err.value)
        # ... nor is the reference's text the scaffolds'
        eng.synteny_blocks(r, t, pieces=[(c, 0, 39000, 0) for c in range(3)], first=[0, 1, 2, 3], **BLOCKS_KW)
        with pytest.raises(MxError) as err:
            eng.synteny_identity()
        assert err.value.code == EINVAL
        # the handle goes on: the reference as the query, the target as the subject
        eng.synteny_blocks(r, t, **BLOCKS_KW)
        same_identity(eng.synteny_identity(), restated_identity(eng, r, t, pair["rtexts"], pair["ttexts"]))
        with pytest.raises(MxError) as err:
            eng.synteny_identity(max_seg=0)
        assert err.value.code == EINVAL


def test_identity_needs_blocks_and_text(pair, tmp_path):
    from ntjoin_amd.engine import MxError
    eng, r, t = load_pair(pair)
    with eng:
        with pytest.raises(MxError) as err:
            eng.synteny_identity()
        assert err.value.code == EINVAL and "mxg_synteny_blocks" in str(err.value)
        pieces = [(c, 0, len(s), 0) for c, s in enumerate(pair["contigs"])]
        eng.synteny_blocks(t, r, pieces=pieces, first=list(range(len(pieces) + 1)), **BLOCKS_KW)
        with pytest.raises(MxError) as err:   # a table, and nothing kept
            eng.synteny_identity()
        assert err.value.code == EINVAL and "kept no text" in str(err.value)
        eng.synteny_blocks(t, r, **BLOCKS_KW)
        assert eng.synteny_identity()["n_aligned"] > 5000
    with engine() as eng:   # a reference that came as a minimizer table holds no text
        t = eng.add_fasta("tgt", 1.0, pair["tgt"])
        eng.sketch(t)
        tsv = str(tmp_path / "tgt.tsv")
        eng.write_tsv(t, tsv)
        x = eng.add_tsv("from_tsv", 1.0, tsv)
        eng.sketch()
        eng.build_graph()
        lengths = [len(c) for c in pair["contigs"]]
        assert eng.synteny_blocks(t, x, subject_length=lengths, min_anchors=2)["n_blocks"] > 0
        with pytest.raises(MxError) as err:
            eng.synteny_identity()
        assert err.value.code == EINVAL and "does not hold" in str(err.value)


def small_pair(td, n_bases, same):
    rng = random.Random(n_bases)
    a = cases.rand_seq(rng, n_bases)
    b = a if same else cases.rand_seq(rng, n_bases)
    ta = write_fasta(td / "a.fa", [("a", a), ("junk_a", cases.rand_seq(rng, 300))], [60, 60])
    tb = write_fasta(td / "b.fa", [("b", b), ("junk_b", cases.rand_seq(rng, 300))], [80, 80])
    eng = engine()
    x, y = eng.add_fasta("a", 1.0, str(td / "a.fa")), eng.add_fasta("b", 1.0, str(td / "b.fa"))
    eng.sketch()
    eng.build_graph()
    return eng, x, y, ta, tb


def test_no_block_and_one_block(tmp_path):
    eng, x, y, ta, tb = small_pair(tmp_path, 2000, same=False)
    with eng:
        assert eng.synteny_blocks(y, x, **BLOCKS_KW)["n_blocks"] == 0
        got = eng.synteny_identity()
        assert all(got[n] == 0 for n in R.SUM_FIELDS) and all(len(got["blocks"][n]) == 0 for n in R.BLOCK_FIELDS)
        eng.write_synteny_paf(tmp_path / "none.paf", identity=True)
        assert (tmp_path / "none.paf").read_bytes() == b""
    eng, x, y, ta, tb = small_pair(tmp_path, 2000, same=True)
    with eng:
        blk = eng.synteny_blocks(y, x, **BLOCKS_KW)
        assert blk["n_blocks"] == 1
        got = eng.synteny_identity()
        same_identity(got, restated_identity(eng, y, x, tb, ta))
        n = int(blk["n_anchors"][0])
        assert (got["n_segments"], got["n_aligned"], got["edits"], got["n_saturated"]) == (n, n, 0, 0)
        assert got["aligned_q"] == got["aligned_s"] == got["block_q"] == int(blk["q_end"][0]) - int(blk["q_start"][0])


def test_a_block_of_4097_anchors(tmp_path):
    "through the scaffolds' table: the first node of a path ends behind the 4097th anchor of its record, the second shares nothing"
    eng, x, y, ta, tb = small_pair(tmp_path, 40000, same=True)
    with eng:
        g = eng.get_graph()
        pos = sorted(int(p) for p, rec in zip(g["vertex_pos"][y], g["vertex_record"][y]) if rec == 0)
        assert len(pos) > 4200
        end = pos[4096] + K
        fa, ufa = tmp_path / "assigned.fa", tmp_path / "unassigned.fa"
        eng.write_scaffolds(y, [(0, 0, end, 3, 0, 0, 0), (1, 0, 300, 0, 0, 0, 1)], [0, 2], assigned=fa, unassigned=ufa, keep=True)
        scaf = parse_fasta(fa)[1] + parse_fasta(ufa)[1]
        pieces, first, _ids = eng.scaffold_pieces()
        blk = eng.synteny_blocks(y, x, pieces=pieces, first=first, **BLOCKS_KW)
        assert blk["n_anchors"].tolist()[0] == 4097 and blk["n_blocks"] == 2
        got = eng.synteny_identity()
        same_identity(got, restated_identity(eng, y, x, scaf, ta, pieces=pieces, first=first))
        assert int(got["blocks"]["n_aligned"][0]) == 4097 and got["edits"] == 0 and got["aligned_q"] == got["block_q"]


@pytest.mark.parametrize("win", ["1", "7", "4096"])
def test_paf_tags_in_small_windows(win, pair, tmp_path, monkeypatch):
    "MXG_SYN_WIN: bytes of PAF text per device window, parsed once per handle: a fresh handle each time"
    def run(name):
        if win == "1":   # (one launch per byte: a short text)
            eng, x, y, _ta, _tb = small_pair(tmp_path, 2000, same=True)
            q, s = y, x
        else:
            eng, s, q = load_pair(pair)
        with eng:
            # (windows of 4096 bytes: links of at most 25 bases, so that every lost minimizer ends a block and the text has many lines)
            eng.synteny_blocks(q, s, **dict(BLOCKS_KW, max_gap=25 if win == "4096" else 100000))
            got = eng.synteny_identity()
            eng.write_synteny_paf(tmp_path / (name + "_plain.paf"))
            eng.write_synteny_paf(tmp_path / (name + ".paf"), identity=True)
            knobs = eng.knobs()
        return (tmp_path / (name + ".paf")).read_bytes(), paf_with_tags((tmp_path / (name + "_plain.paf")).read_bytes(), got), knobs
    default, want, _ = run("default")
    assert default == want and b"\tNM:i:" in default and b"\tdv:f:0." in default
    monkeypatch.setenv("MXG_SYN_WIN", win)
    got, want, knobs = run("win")
    assert got == default == want and len(got) > 3 * int(win)
    assert f"MXG_SYN_WIN={win}" in knobs


def test_lanes_in_list_order_give_the_same(pair, monkeypatch):
    "MXG_IDY_ORDER=0: the segments dealt to the lanes in list order, without the radix sort by falling length that is the default"
    eng, r, t = load_pair(pair)
    with eng:
        eng.synteny_blocks(t, r, **BLOCKS_KW)
        want = eng.synteny_identity()
        assert "MXG_IDY_ORDER" not in eng.knobs()
    monkeypatch.setenv("MXG_IDY_ORDER", "0")
    eng, r, t = load_pair(pair)
    with eng:
        eng.synteny_blocks(t, r, **BLOCKS_KW)
        got = eng.synteny_identity()
        assert "MXG_IDY_ORDER=0" in eng.knobs()
        assert {n: got[n] for n in R.SUM_FIELDS} == {n: want[n] for n in R.SUM_FIELDS} and want["n_aligned"] > 5000
        assert all(got["blocks"][n].tolist() == want["blocks"][n].tolist() for n in R.BLOCK_FIELDS)
        small = eng.synteny_identity(max_seg=20)
        same_identity(small, restated_identity(eng, t, r, pair["ttexts"], pair["rtexts"], max_seg=20))
