"""GPU tests of the FASTA index route (ntjoin_amd/csrc/fai.hip): mxg_write_fai against the two `samtools faidx` outputs the reference
records (tests/golden/fai/) and, on every other input, against the restatement of its contract (tests/_fai_restatement.py): the
shapes and refusals of tests/_fai_cases.py, assemblies without text, small windows, duplicate names, BGZF input with its .gzi;
MXG_SCAF_FAI on the goldens and fuzz seeds of the scaffold stage; and both routes past the borders of their scans: one long record
on the tile and round borders of the scan over the work items (256 items, 65 536 items), the rows' offsets around 1 024 and
262 144 entries of the shared 64-bit scan."""
import functools
import glob
import os
import random
import re
import zlib

import pytest

from ntjoin_amd import fai as fai_mod
from ntjoin_amd.engine import MxEngine, MxError
from tests import _bgzf, _fai_cases, _fai_restatement as R, _oracle, _scaffold_cases as cases
from tests.conftest import GOLDEN
from tests.test_fai_cpu import carry_place, carry_want, check_fetch

pytestmark = pytest.mark.gpu
EINVAL = -1
KNOBS = ("MXG_FAI_WIN", "MXG_HOST_INGEST", "MXG_BGZF_PAYLOAD", "MXG_SCAF_WIN", "MXG_DEBUG_IO")
SHAPES = _fai_cases.shapes()
REFUSALS = _fai_cases.refusals()


@pytest.fixture
def env():
    saved = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    yield os.environ
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


def index_files(tmp_path, texts, **kw):
    "every text as an assembly of handles of up to 30 -> {name: the .fai's bytes, or the MxError}"
    out, names = {}, sorted(texts)
    for lo in range(0, len(names), 30):
        with MxEngine(k=15, w=10, **kw) as eng:
            for name in names[lo:lo + 30]:
                fa = tmp_path / (name + ".fa")
                fa.write_bytes(texts[name])
                a = eng.add_fasta(name, 1.0, str(fa))
                try:
                    eng.write_fai(a, str(fa) + ".fai")
                    out[name] = read(str(fa) + ".fai")
                except MxError as err:
                    assert not os.path.exists(str(fa) + ".fai")
                    out[name] = err
    return out


def test_goldens(env, tmp_path):
    texts = {name: read(os.path.join(GOLDEN, "fasta", name)) for name in sorted(os.listdir(os.path.join(GOLDEN, "fasta")))}
    got = index_files(tmp_path, texts)
    for name in ("ref.fa", "scaf.f-f.fa"):
        assert got[name] == read(os.path.join(GOLDEN, "fai", name + ".fai"))
    for name, text in texts.items():
        assert got[name] == R.fai_bytes(text), name
    assert b"\t70\t71\n" in got["synth.tgt.fa"]


def test_shapes(env, tmp_path):
    got = index_files(tmp_path, SHAPES)
    for name, text in SHAPES.items():
        assert not isinstance(got[name], MxError), (name, got[name])
        assert got[name] == R.fai_bytes(text), name
        check_fetch(R.parse(got[name]), text, tries=6)


def test_refusals(env, tmp_path):
    "MXG_EINVAL with the record's id in the message, nothing at the path, and the handle goes on"
    good = SHAPES["headers"]
    names = sorted(REFUSALS)
    for lo in range(0, len(names), 28):
        with MxEngine(k=15, w=10) as eng:
            for name in names[lo:lo + 28]:
                text, bad = REFUSALS[name]
                fa = tmp_path / (name + ".fa")
                fa.write_bytes(text)
                a = eng.add_fasta(name, 1.0, str(fa))
                with pytest.raises(MxError) as err:
                    eng.write_fai(a, str(fa) + ".fai")
                assert err.value.code == EINVAL and "record '%s'" % bad in str(err.value), name
                assert not os.path.exists(str(fa) + ".fai")
            fa = tmp_path / "good.fa"
            fa.write_bytes(good)
            a = eng.add_fasta("good", 1.0, str(fa))
            eng.write_fai(a, str(fa) + ".fai")
            assert read(str(fa) + ".fai") == R.fai_bytes(good)


def test_no_text_held(env, tmp_path):
    fa = tmp_path / "t.fa"
    fa.write_bytes(read(os.path.join(GOLDEN, "fasta", "scaf.f-f.fa")))
    out = str(tmp_path / "t.fai")

    def refused(eng, a, match="does not hold"):
        with pytest.raises(MxError) as err:
            eng.write_fai(a, out)
        assert err.value.code == EINVAL and match in str(err.value) and not os.path.exists(out)

    with MxEngine(k=32, w=100) as eng:
        a = eng.add_fasta("t", 1.0, str(fa))
        eng.sketch(a)
        tsv = str(tmp_path / "t.tsv")
        eng.write_tsv(a, tsv)
        with pytest.raises(MxError) as err:  # a .gzi for plain text
            eng.write_fai(a, out, gzi=out + ".gzi")
        assert err.value.code == EINVAL and "BGZF" in str(err.value) and not os.path.exists(out) and not os.path.exists(out + ".gzi")
        refused(eng, eng.add_tsv("from_tsv", 1.0, tsv))
        eng.write_fai(a, out)  # (the handle goes on)
        assert read(out) == read(os.path.join(GOLDEN, "fai", "scaf.f-f.fa.fai"))
        os.remove(out)
    env["MXG_HOST_INGEST"] = "1"
    with MxEngine(k=32, w=100) as eng:
        refused(eng, eng.add_fasta("t", 1.0, str(fa)))
    del env["MXG_HOST_INGEST"]
    with MxEngine(k=32, w=100, drop_seq=True) as eng:
        refused(eng, eng.add_fasta("t", 1.0, str(fa)))


def _digit_border_fasta():
    "more than 300 records whose lengths and offsets cross every digit border from 1 to 7 digits"
    rng = random.Random(9)
    lens = [1, 9, 10, 11, 99, 100, 101, 999, 1000, 1001, 9999, 10000, 10001, 99999, 100000, 100001, 999999, 1000000, 1000001]
    recs = [(n, rng.choice([60, 70, 0])) for n in [1] * 3 + [2, 3, 9, 10, 30] * 8 + [rng.randint(1, 400) for _ in range(260)] + lens]
    parts = []
    for i, (n, w) in enumerate(recs):
        s = (_fai_cases.seq(rng, 1000) * (n // 1000 + 1))[:n]
        head = _fai_cases.header("r%d" % i, " len %d" % n) if i else _fai_cases.header("a")  # (the first text starts at byte 3)
        parts.append(head + _fai_cases.fold(s, w or n))
    return "".join(parts).encode()


def test_windows(env, tmp_path):
    text = _digit_border_fasta()
    want = R.fai_bytes(text)
    rows = R.parse(want)
    assert len(rows) >= 300
    for col in (1, 2):  # lengths and offsets: every digit count from 1 to 7
        assert {len(str(r[col])) for r in rows} >= set(range(1, 8))
    fa = tmp_path / "d.fa"
    fa.write_bytes(text)
    for win in (None, "1", "7", "4093"):
        if win:
            env["MXG_FAI_WIN"] = win
        with MxEngine(k=15, w=10) as eng:  # (a knob is read once per handle)
            a = eng.add_fasta("d", 1.0, str(fa))
            eng.write_fai(a, str(tmp_path / "d.fai"))
            assert (f"MXG_FAI_WIN={win}" in eng.knobs()) == bool(win)
        assert read(str(tmp_path / "d.fai")) == want, win


def test_duplicate_names(env, tmp_path, capfd):
    text = _fai_cases.duplicates()
    rows, dropped = R.index(text)
    fa = tmp_path / "dup.fa"
    fa.write_bytes(text)
    with MxEngine(k=15, w=10) as eng:
        a = eng.add_fasta("dup", 1.0, str(fa))
        capfd.readouterr()
        eng.write_fai(a, str(fa) + ".fai")
    lines = [ln for ln in capfd.readouterr().err.splitlines() if "duplicate" in ln]
    assert read(str(fa) + ".fai") == R.format_rows(rows)
    assert len(lines) == len(dropped) == 3 and all('"%s"' % name in ln for name, ln in zip(dropped, lines))


def members_of(blob):
    "[(compressed offset, text offset)] of the members that hold text, by the members' own headers"
    from tests.test_fai_cpu import _bgzf_members_of
    return _bgzf_members_of(blob)[1]


def check_random_access(blob, gzi, text, seed=3, tries=50):
    "for random text offsets: the last pair at or below it (or the file's start), that one member inflated, the bytes compared"
    pairs = [(0, 0)] + R.parse_gzi(gzi)
    assert pairs == sorted(pairs)
    rng = random.Random(seed)
    for _ in range(tries):
        at = rng.randrange(len(text))
        c, u = [p for p in pairs if p[1] <= at][-1]
        (xlen,) = (int.from_bytes(blob[c + 10:c + 12], "little"),)
        bsize = int.from_bytes(blob[c + 16:c + 18], "little")
        assert blob[c:c + 4] == b"\x1f\x8b\x08\x04"
        got = zlib.decompress(blob[c + 12 + xlen:c + bsize + 1 - 8], -15)
        assert u + len(got) > at and got == text[u:u + len(got)]


def test_bgzf_input(env, tmp_path):
    text = SHAPES["widths_crlf_short_noeol"]
    fa, gz = tmp_path / "p.fa", tmp_path / "z.fa.gz"
    fa.write_bytes(text)
    _bgzf.write_bgzf(str(gz), text, [65280, 1, 4096, 0, 30000])
    blob = read(str(gz))
    with MxEngine(k=15, w=10) as eng:
        a, z = eng.add_fasta("p", 1.0, str(fa)), eng.add_fasta("z", 1.0, str(gz))
        eng.write_fai(a, str(fa) + ".fai")
        eng.write_fai(z, str(gz) + ".fai", gzi=str(gz) + ".gzi")
    assert read(str(gz) + ".fai") == read(str(fa) + ".fai") == R.fai_bytes(text)
    gzi = read(str(gz) + ".gzi")
    assert gzi == R.gzi_bytes(members_of(blob))
    check_random_access(blob, gzi, text)


# ---- MXG_SCAF_FAI
GOLDENS = sorted(glob.glob(os.path.join(cases.GOLDEN, "scaffolds", "*.json")))
SCAF_CASES = [("fuzz", s) for s in cases.FUZZ_SEEDS] + [("golden", g) for g in GOLDENS]
SCAF_IDS = [f"fuzz{s}" for s in cases.FUZZ_SEEDS] + [os.path.basename(g)[:-5] for g in GOLDENS]


def scaffold_inputs(kind, which, tmp_path):
    if kind == "fuzz":
        case = cases.fuzz_case(which)
        fasta = str(tmp_path / "t.fa")
        cases.write_fasta(fasta, case["records"], case["width"], case["final_newline"])
        return case["records"], case["paths"], case["overlap_gap"], case["fold"], fasta
    doc, fasta = cases.load_golden(which)
    return _oracle.read_fasta(fasta), cases.golden_nodes(doc), doc["meta"]["overlap_gap"] if doc["meta"]["overlap"] else None, False, fasta


def scaffolds(eng, a, records, paths, out, overlap_gap, fold, **kw):
    index = {rid: r for r, (rid, _) in enumerate(records)}
    rows, first = cases.rows_of(paths, index)
    names = [str(out) + s for s in (".assigned.fa", ".unassigned.fa", ".bed")]
    res = eng.write_scaffolds(a, rows, first, overlap_gap=overlap_gap, fold_case=fold, assigned=names[0], unassigned=names[1], bed=names[2], **kw)
    return names, (res["lead_strip"].tolist(), res["tail_strip"].tolist(), res["n_unassigned"])


def check_scaffold_indexes(kind, which, tmp_path, k, w):
    "plain, with the .fai, and as BGZF with .fai and .gzi: the same FASTA and BED; the indexes equal the restatement over the plain files"
    records, paths, gap, fold, fasta = scaffold_inputs(kind, which, tmp_path)
    with MxEngine(k=k, w=w) as eng:
        a = eng.add_fasta("t", 1.0, fasta)
        plain, res0 = scaffolds(eng, a, records, paths, tmp_path / "plain", gap, fold)
        for n in plain[:2]:
            assert not os.path.exists(n + ".fai") and not os.path.exists(n + ".gzi")
        fai, res1 = scaffolds(eng, a, records, paths, tmp_path / "fai", gap, fold, fai=True)
        comp, res2 = scaffolds(eng, a, records, paths, tmp_path / "comp", gap, fold, fai=True, bgzf=True)
    assert res0 == res1 == res2
    assert [read(n) for n in fai] == [read(n) for n in plain] and read(comp[2]) == read(plain[2])
    n_lines = []
    for p, f, c in zip(plain[:2], fai[:2], comp[:2]):
        text = read(p)
        want = R.fai_bytes(text)
        assert read(f + ".fai") == want and read(c + ".fai") == want and not os.path.exists(f + ".gzi")
        assert text.count(b">") == want.count(b"\n")  # (an interval dropped from the FASTA has no line)
        blob, gzi = read(c), read(c + ".gzi")
        assert gzi == R.gzi_bytes(members_of(blob))
        if text:
            check_random_access(blob, gzi, text, tries=50)
        n_lines.append(want.count(b"\n"))
    assert n_lines[1] == res0[2]
    # the two BGZF files as `ntJoin-mx scaffold gz=True` joins them, and the index of the whole from those of its parts
    whole = str(tmp_path / "all.fa.gz")
    with open(whole, "wb") as fh:
        fh.write(read(comp[0])[:-28] + read(comp[1]))
    fai_mod.cat_files(comp[0], comp[1], whole)
    text = read(plain[0]) + read(plain[1])
    assert read(whole + ".fai") == R.fai_bytes(text)
    assert read(whole + ".gzi") == R.gzi_bytes(members_of(read(whole)))
    check_random_access(read(whole), read(whole + ".gzi"), text, tries=50)
    return n_lines


@pytest.mark.parametrize("kind,which", SCAF_CASES, ids=SCAF_IDS)
def test_scaffold_indexes(kind, which, env, tmp_path):
    k, w = (15, 10) if kind == "fuzz" else (32, 100)
    check_scaffold_indexes(kind, which, tmp_path, k, w)


@pytest.mark.parametrize("seed", [2, 7, 19])
def test_scaffold_indexes_with_borders_inside_records(seed, env, tmp_path):
    "members of 255 bytes and windows of one emit tile: member and window borders fall inside records"
    env["MXG_BGZF_PAYLOAD"] = "255"
    env["MXG_SCAF_WIN"] = "8192"
    env["MXG_FAI_WIN"] = "64"
    check_scaffold_indexes("fuzz", seed, tmp_path, 15, 10)


# ---- the carries: the scan over the work items, and the offset scan at 1 024 and 262 144 entries
B = _fai_cases.ITEMS_ROUND


def indexed(env, tmp_path, capfd, text, win=None):
    "-> (the .fai's bytes or the MxError, the items the witness line of MXG_DEBUG_IO names)"
    env["MXG_DEBUG_IO"] = "1"
    if win:
        env["MXG_FAI_WIN"] = win
    fa = tmp_path / "c.fa"
    fa.write_bytes(text)
    out = str(fa) + ".fai"
    if os.path.exists(out):
        os.remove(out)
    with MxEngine(k=15, w=10) as eng:
        a = eng.add_fasta("c", 1.0, str(fa))
        capfd.readouterr()
        try:
            eng.write_fai(a, out)
            got = read(out)
        except MxError as err:
            assert not os.path.exists(out)
            got = err
        assert (f"MXG_FAI_WIN={win}" in eng.knobs()) == bool(win)
    witness = re.findall(r"^\[mxg\] fai items=(\d+) rows_ms=", capfd.readouterr().err, re.M)
    assert len(witness) == 1
    return got, int(witness[0])


@pytest.mark.parametrize("name", sorted(_fai_cases.CARRIES))
def test_row_scan_carries(name, env, tmp_path, capfd):
    """"long" on the borders of k_fai_tile_scan's tiles and rounds (tests/test_fai_cpu.py says which fault each case is there for):
    the file is the restatement's, or the refusal names the record and the restatement's byte; the items are the cutting rule's"""
    kw, refused = _fai_cases.CARRIES[name]
    text = _fai_cases.carry_case(name)
    at, span, total = carry_place(name)
    assert (at, span) == (kw["at"], kw["span"])  # (a builder that drifts fails here, not in the coverage)
    status, want = carry_want(name)
    got, n_items = indexed(env, tmp_path, capfd, text)
    assert n_items == total
    if name.startswith("exact"):
        assert n_items == (B if name == "exact_round" else B + 1)
    if refused:
        with pytest.raises(R.Refused) as ref:
            R.index(text)
        assert status == 3 and isinstance(got, MxError) and got.code == EINVAL
        assert "record 'long'" in str(got) and "the line at byte %d of the text" % ref.value.offset in str(got)
        return
    assert status == 0 and not isinstance(got, MxError), got
    assert got == want
    if name == "across":
        rows = R.parse(got)
        at_row = [row[0] for row in rows].index("long")
        check_fetch(rows[:3] + rows[at_row - 3:at_row + 4] + rows[-3:], text, tries=6)


OFFSET_DUP = (500, 100000)  # records that bear the name in front of them: no line, a size of 0 inside the scan


@functools.lru_cache(maxsize=None)
def offset_case(n):
    "(text, the index by the restatement, items) of n tiny records"
    text = _fai_cases.tiny_records(n, tuple(d for d in OFFSET_DUP if d < n))
    rows, dropped = R.index(text)
    assert len(rows) + len(dropped) == n and len(dropped) == sum(d < n for d in OFFSET_DUP)
    assert len({len(R.format_rows([row])) for row in rows[:1024]}) >= 8  # (the sizes under the scan differ)
    return text, R.format_rows(rows), sum(_fai_cases.items_of(text))


@pytest.mark.parametrize("n,win", [(1022, None), (1023, None), (1024, None), (262143, None), (262143, "4093"), (262144, None), (262144, "4093")])
def test_offset_scan_borders(n, win, env, tmp_path, capfd):
    """n + 1 row sizes on either side of a tile (1 024) and of a round (262 144) of the 64-bit scan, a kept-out row in the first tile
    and in the first round; with windows of 4093 bytes k_win_bounds bisects offsets that live on the round carry"""
    text, want, items = offset_case(n)
    got, n_items = indexed(env, tmp_path, capfd, text, win)
    assert not isinstance(got, MxError), got
    assert n_items == items and items >= n
    if n >= 4 * B:
        assert n_items > 4 * B  # (a fifth round of the scan over the items as well)
    assert got == want


SCAF_RECORDS, SCAF_PATHS = 262150 + 2200, 1100
fai_of_text = functools.lru_cache(maxsize=None)(R.fai_bytes)  # (both runs write the same two plain files)


@pytest.mark.parametrize("bgzf", [False, True], ids=["plain", "bgzf"])
def test_scaffold_indexes_past_the_scan_borders(bgzf, env, tmp_path):
    """1 100 scaffolds of two records (ntJoin<i> rows past the tile border of both scans of write_fai_records) and 262 150 and more
    unassigned records (id:lo-hi rows past the round border); as check_scaffold_indexes: the index of each file is the restatement's
    over the plain file the same handle wrote, FASTA and BED do not change"""
    recs = [("c%d%s" % (i, "y" * (i // 41 % 19)), ("ACGTTGCA" * 6)[i % 8:i % 8 + 9 + i % 31]) for i in range(SCAF_RECORDS)]
    fasta = str(tmp_path / "t.fa")
    cases.write_fasta(fasta, recs, 0)
    rows, first = [], [0]
    for p in range(SCAF_PATHS):
        a, b = 2 * p, 2 * p + 1
        cut = 2 if p % 10 == 0 else 0  # (some nodes leave the record's first bases unassigned: id:0-2)
        rows += [(a, cut, len(recs[a][1]), 3 + p % 5, 0, 0, p % 3 == 1), (b, 0, len(recs[b][1]), 0, 0, 0, p % 2 == 1)]
        first.append(len(rows))
    with MxEngine(k=15, w=10) as eng:
        asm = eng.add_fasta("t", 1.0, fasta)
        outs = []
        for tag, kw in (("plain", {}), ("idx", dict(fai=True, bgzf=bgzf))):
            names = [str(tmp_path / tag) + s for s in (".assigned.fa", ".unassigned.fa", ".bed")]
            res = eng.write_scaffolds(asm, rows, first, assigned=names[0], unassigned=names[1], bed=names[2], **kw)
            outs.append((names, (res["lead_strip"].tolist(), res["tail_strip"].tolist(), res["n_unassigned"])))
    (plain, res0), (idx, res1) = outs
    assert res0 == res1 and read(idx[2]) == read(plain[2])
    n_lines = []
    for p, f in zip(plain[:2], idx[:2]):
        text = read(p)
        assert not os.path.exists(p + ".fai")
        want = fai_of_text(text)
        assert read(f + ".fai") == want
        assert text.count(b">") == want.count(b"\n")
        n_lines.append(want.count(b"\n"))
        if bgzf:
            blob, gzi = read(f), read(f + ".gzi")
            assert gzi == R.gzi_bytes(members_of(blob))
            check_random_access(blob, gzi, text, tries=20)
        else:
            assert read(f) == text and not os.path.exists(f + ".gzi")
    assert n_lines[0] == SCAF_PATHS > 1025 and n_lines[1] == res0[2] > 262145
