"""GPU tests of the reference-based stages -- mxg_synteny_blocks, mxg_write_synteny_paf(_ex), mxg_synteny_assess, mxg_synteny_identity,
mxg_identity_segments (include/ntjoin_mx.h, rows f12 .. f14) -- at MANY RECORDS: 1 to 65 537 subject records and 255 to 65 537 query
records (tests/_many_records.py), against the sequential restatements (tests/_synteny_restatement.py, tests/_assess_restatement.py,
tests/_identity_restatement.py).  Every comparison is exact.

What the record counts reach: the sort of the chains by s_record << 32 | s_start in assess.hip on its five-, six- and seven-pass
routes (up to 255, up to 65 535, from 65 536 subject records) and with it the buffer its result lies in; the running maximum of
s_record << 32 | s_end with a record border at nearly every element and record numbers of 2^16 and more in its upper half; the ng
figures over far more record lengths than chains, also where no block is kept; piece tables, the PAF writer's name offsets and its
windows over 65 537 records; and, for the identity, contigs shorter than an ingest tile, so that every tile and nearly half of the 256-byte
sub-tiles hold the end of one record and the start of the next.  An eight-pass sort takes 2^24 subject records, which no test of a few
seconds builds: it is not tested.  tests/test_many_records_cpu.py asserts without a GPU that the cases are what they are said to
be here, and that a sort of a pass too few changes covered_subject of the subject cases."""
import pytest

from tests import _assess_restatement as A, _identity_restatement as IR, _many_records as MR, _synteny_restatement as R
from tests.test_gpu_assess import check as check_assess
from tests.test_gpu_identity import BLOCKS_KW, K as IDY_K, check as check_segments, engine, parse_fasta, paf_with_tags, restated_identity, same_identity
from tests.test_gpu_synteny import as_tuples, check as check_blocks, load, write_paf

pytestmark = pytest.mark.gpu

ZEROS = dict(n50=0, l50=0, n75=0, l75=0, n90=0, l90=0)


# ---- 1: subject records -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_s", MR.COUNTS)
def test_subject_record_counts_across_the_sort_s_passes(n_s):
    """a chain per block, on subject records in shuffled order (tests/_many_records.py::many_subject_case): scalars, chains and
    breakpoints; with merge_gap = 100; and, for 256 and 65 537 records, once more after a call whose subject has two records"""
    case = MR.cached("many_subject_case", n_s)
    again = n_s in (256, 65537)
    loaded = MR.with_two_record_subject(case) if again else case
    n = MR.subject_blocks(n_s)
    with load(loaded) as eng:
        if n_s <= 257:   # (at 65 537 records the blocks are compared by the PAF test below)
            assert len(check_blocks(eng, loaded)["blocks"]) == n
        nx = dict(lengths=case["nx_lengths"] + loaded["lengths"][2:])   # (see many_subject_case: lengths that let the Nx figures reach 50 %)
        blocks, want = check_assess(eng, loaded, **nx)
        assert blocks["n_blocks"] == want["n_chains"] == n and len(set(want["chains"]["s_record"])) == n_s
        assert want["covered_subject"] < want["chained_subject"]
        assert want["na"]["l50"] > 0 and want["nga"]["l50"] > 0 and want["ng"]["l50"] > 0
        assert want["n_breakpoints"] == n - 1 and sum(want["breakpoints"].values()) == n - 1
        if n_s >= 127:
            assert want["breakpoints"][(A.TRANSLOCATION, 0)] > 0.98 * n
        _, merged = check_assess(eng, loaded, assess=dict(merge_gap=100), **nx)
        assert merged["n_chains"] == n
        if again:
            small, _ = check_assess(eng, loaded, s=2)
            assert small["n_blocks"] == n and set(small["s_record"].tolist()) == {0, 1}
            _, once_more = check_assess(eng, loaded, **nx)
            assert once_more == want


# ---- 2: query records -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_q", MR.QUERY_COUNTS)
def test_query_record_counts(n_q):
    "a block, and so a chain, on every query record; ng over n_q lengths of 47 values"
    case = MR.cached("many_query_case", n_q)
    with load(case) as eng:
        assert len(check_blocks(eng, case)["blocks"]) == n_q
        _, want = check_assess(eng, case)
    assert want["n_chains"] == n_q and want["n_breakpoints"] == 0
    assert want["na"]["l50"] > 0 and want["nga"]["l50"] > 0 and want["ng"]["l90"] > want["ng"]["l50"] > 0


@pytest.mark.parametrize("n_q", [1025, 65537])
def test_far_more_query_records_than_chains(n_q):
    """three chains among n_q query records, most of them without a minimizer.  On a fresh handle the first call keeps no block
    (min_anchors = 3): the lengths alone size the buffers of the sort; then the three chains; then no block again"""
    case = MR.cached("few_chains_case", n_q)
    with load(case) as eng:
        for min_anchors in (3, 2, 3):
            blocks, want = check_assess(eng, case, min_anchors=min_anchors)
            assert want["ng"]["l50"] > n_q // 4 and want["ng"]["l90"] > want["ng"]["l50"]
            if min_anchors == 3:
                assert blocks["n_blocks"] == want["n_chains"] == want["aligned_query"] == want["covered_subject"] == 0
                assert want["na"] == want["nga"] == ZEROS
            else:
                assert blocks["n_blocks"] == 6 and want["n_chains"] == 3 and want["chains"]["q_record"] == [0, n_q // 2, n_q - 1]


@pytest.mark.parametrize("name", sorted(MR.TABLES))
def test_piece_tables_over_65537_source_records(name):
    """a piece per record, every other one REV; those pieces dealt into table records of 1 to 40 with GAP pieces between them; only the
    records from 256 on, in falling order: the blocks, then chains and breakpoints (at_join through the table's offsets)"""
    case = MR.cached("many_query_case", 65537)
    pieces, first = MR.TABLES[name](case)
    with load(case) as eng:
        n_blocks = len(check_blocks(eng, case, pieces=pieces, first=first)["blocks"])
        _, want = check_assess(eng, case, pieces=pieces, first=first)
    assert want["n_chains"] == n_blocks == (65537 - 256 if name == "high_falling" else 65537)
    joins = sum(want["breakpoints"][(kind, 1)] for kind in range(3))
    assert joins == want["n_breakpoints"] and (joins > 60000) == (name == "dealt") and want["ng"]["l50"] > 0


# ---- 3: PAF ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", [None, "4096"])
@pytest.mark.parametrize("builder", ["many_subject_case", "many_query_case"])
def test_paf_over_65537_records(builder, win, tmp_path, monkeypatch):
    """byte for byte against the restatement: the subject's names are the handle's (rec0 .. rec65536), the query's the caller's, of 1
    to 40 bytes.  At the default window the text is written twice, the second time with append; MXG_SYN_WIN is parsed once per
    handle, so the small window has a handle of its own"""
    case = MR.paf_case(MR.cached(builder, 65537))
    n_blocks = MR.subject_blocks(65537) if builder == "many_subject_case" else 65537
    if win is None:
        got, want, knobs = write_paf(case, tmp_path / "twice.paf", n_refs=2)
        assert "MXG_SYN_WIN" not in knobs and got.count(b"\n") == 2 * n_blocks and got[:len(got) // 2] == got[len(got) // 2:]
    else:
        monkeypatch.setenv("MXG_SYN_WIN", win)
        got, want, knobs = write_paf(case, tmp_path / "win.paf")
        assert f"MXG_SYN_WIN={win}" in knobs and got.count(b"\n") == n_blocks
    assert got == want and len(got) > 3_000_000


# ---- 4: identity over contigs shorter than a tile ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def short(tmp_path_factory):
    files = MR.short_contig_files(tmp_path_factory.mktemp("short_contigs"))
    data = open(files["tgt"], "rb").read()
    inside, shared, tiles = MR.tile_counts(data, MR.TILE)
    # every 4096-byte tile of the target holds bytes of two records or more (a contig has at most 900 bases) ...
    assert shared == tiles >= 35 and inside >= 30
    # ... and of the 256-byte sub-tiles, whose first one of a record is where text_of_base clamps its scan, at least 250 do; at
    # least 250 of their borders fall inside a record (a file of 150 kbp has fewer than 40 tiles of 4096 bytes)
    inside, shared, _ = MR.tile_counts(data, MR.SUB_TILE)
    assert inside >= 250 and shared >= 250
    return files


def load_short(short):
    eng = engine()
    r, t = eng.add_fasta("ref", 2.0, short["ref"]), eng.add_fasta("tgt", 1.0, short["tgt"])
    eng.sketch()
    eng.build_graph()
    return eng, r, t


def blocks_identity_paf(eng, q, s, qtexts, stexts, tmp_path, q_ids, s_ids):
    "blocks against the restatement's PAF text, identity against the DP, the tagged PAF against the plain one and the tags' formatter"
    blk = eng.synteny_blocks(q, s, **BLOCKS_KW)
    got = eng.synteny_identity()
    same_identity(got, restated_identity(eng, q, s, qtexts, stexts))
    eng.write_synteny_paf(tmp_path / "plain.paf")
    eng.write_synteny_paf(tmp_path / "tags.paf", identity=True)
    plain = (tmp_path / "plain.paf").read_bytes()
    kept = list(zip(*[blk[name].tolist() for name in R.FIELDS]))
    assert plain.decode() == R.paf(kept, q_ids, [len(IR.bases(t)) for t in qtexts], s_ids, [len(IR.bases(t)) for t in stexts], IDY_K)
    assert (tmp_path / "tags.paf").read_bytes() == paf_with_tags(plain, got)
    return blk, got


def test_short_contigs_as_the_query(short, tmp_path):
    "300 query records"
    eng, r, t = load_short(short)
    with eng:
        blk, got = blocks_identity_paf(eng, t, r, short["ttexts"], short["rtexts"], tmp_path, [f"ctg{c}" for c in range(300)], ["chr0", "chr1", "chr2"])
    assert len(set(blk["q_record"].tolist())) >= 290 and got["n_blocks"] >= 290 and 15000 < got["n_segments"] < 40000
    assert got["n_skip_n"] >= 1 and got["n_aligned"] > 15000 and 0 < got["edits"] < got["aligned_q"] // 20 and any(blk["reverse"])


def test_short_contigs_as_the_subject(short, tmp_path):
    "300 subject records, whose streams run backwards for the reverse blocks"
    eng, r, t = load_short(short)
    with eng:
        blk, got = blocks_identity_paf(eng, r, t, short["rtexts"], short["ttexts"], tmp_path, ["chr0", "chr1", "chr2"], [f"ctg{c}" for c in range(300)])
    assert len(set(blk["s_record"].tolist())) >= 290 and got["n_aligned"] > 15000 and 0 < got["edits"] < got["aligned_q"] // 20
    backwards = {int(sr) for sr, rev in zip(blk["s_record"], blk["reverse"]) if rev}
    assert len(backwards & set(range(1, 300, 3))) >= 90   # (every third contig is reverse-complemented)


def test_ends_of_every_short_contig(short):
    """mxg_identity_segments: of every target record its first 40 bases, its last 40, its first base and its last base against the
    same interval of the same file, forward (no edit) and with the subject side reversed (whatever the DP says)"""
    segs = []
    for c, seq in enumerate(short["contigs"]):
        n = len(seq)
        for at, ln in ((0, 40), (n - 40, 40), (0, 1), (n - 1, 1)):
            segs += [(c, at, ln, c, at, ln, 0), (c, at, ln, c, at, ln, 1)]
    with engine() as eng:
        t = eng.add_fasta("tgt", 1.0, short["tgt"])
        got = check_segments(eng, t, t, short["ttexts"], short["ttexts"], segs)
    assert len(got) == 2400 and all(g == (0, IR.ALIGNED, 0) for g in got[0::2])
    assert all(g[1] == IR.ALIGNED for g in got) and sum(1 for g in got[1::2] if g[0] > 0) > 1000


def test_short_contigs_through_the_kept_scaffold_text(short, tmp_path):
    "one path over contigs 298 and 299 (the second reversed, a gap between them), the other 298 unassigned"
    eng, r, t = load_short(short)
    n = [len(c) for c in short["contigs"]]
    with eng:
        fa, ufa = tmp_path / "assigned.fa", tmp_path / "unassigned.fa"
        eng.write_scaffolds(t, [(298, 0, n[298], 10, 0, 0, 0), (299, 0, n[299], 0, 0, 0, 1)], [0, 2], assigned=fa, unassigned=ufa, keep=True)
        ids, scaf = parse_fasta(fa)
        ids2, scaf2 = parse_fasta(ufa)
        pieces, first, kept_ids = eng.scaffold_pieces()
        assert kept_ids == ids + ids2 and len(ids) == 1 and len(ids2) == 298
        blk = eng.synteny_blocks(t, r, pieces=pieces, first=first, **BLOCKS_KW)
        got = eng.synteny_identity()
        same_identity(got, restated_identity(eng, t, r, scaf + scaf2, short["rtexts"], pieces=pieces, first=first))
    assert got["n_blocks"] == blk["n_blocks"] >= 290 and got["n_aligned"] > 15000 and as_tuples(blk)[0][1] == 0
