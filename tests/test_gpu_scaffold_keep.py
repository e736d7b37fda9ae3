"""GPU tests of MXG_SCAF_KEEP, mxg_scaffold_text, mxg_scaffold_pieces and mxg_scaffold_record_id (csrc/scaffold.hip)
on the goldens and the fuzz seeds of tests/_scaffold_cases.py: with the flag the files are byte for byte what they are without it; the
kept text is the assigned file followed by the unassigned one, also with no file named, under MXG_SCAF_BGZF and with windows of one
tile; the piece table applied to the records of the FASTA spells every kept record; the names are the headers; the refusals."""
import glob
import os

import pytest

from ntjoin_amd import capi
from ntjoin_amd.engine import MxEngine, MxError
from tests import _compose_restatement as R, _oracle, _scaffold_cases as cases
from tests._devmem import download

pytestmark = pytest.mark.gpu

GOLDENS = sorted(glob.glob(os.path.join(cases.GOLDEN, "scaffolds", "*.json")))


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


def golden_case(path):
    doc, fasta = cases.load_golden(path)
    return {"fasta": fasta, "records": _oracle.read_fasta(fasta), "paths": cases.golden_nodes(doc),
            "overlap_gap": doc["meta"]["overlap_gap"] if doc["meta"]["overlap"] else None, "fold": False}


def fuzz_case(seed, tmp_path):
    case = cases.fuzz_case(seed)
    case["fasta"] = str(tmp_path / "t.fa")
    cases.write_fasta(case["fasta"], case["records"], case["width"], case["final_newline"])
    return case


def call(eng, a, case, out, keep, named=True, fold=None, **kw):
    index = {rid: r for r, (rid, _) in enumerate(case["records"])}
    rows, first = cases.rows_of(case["paths"], index)
    names = [str(out) + s for s in (".assigned.fa", ".unassigned.fa", ".bed")] if named else [None, None, None]
    res = eng.write_scaffolds(a, rows, first, overlap_gap=case["overlap_gap"], fold_case=case["fold"] if fold is None else fold,
                              assigned=names[0], unassigned=names[1], bed=names[2], keep=keep, **kw)
    return names, res


def kept(eng):
    addr, n, n_rec = eng.scaffold_text()
    return download(addr, n), n_rec


def check_case(eng, a, case, tmp_path, fold=None):
    fold = case["fold"] if fold is None else fold
    plain, res0 = call(eng, a, case, tmp_path / "plain", keep=False, fold=fold)
    with pytest.raises(MxError) as err:   # (a call without the flag keeps nothing)
        eng.scaffold_text()
    assert err.value.code == capi.MXG_EINVAL
    flagged, res1 = call(eng, a, case, tmp_path / "keep", keep=True, fold=fold)
    for p, q in zip(plain, flagged):
        assert read(p) == read(q), q
    for key in res0:
        assert (res0[key] == res1[key]) if key == "n_unassigned" else (res0[key].tolist() == res1[key].tolist()), key
    want = read(plain[0]) + read(plain[1])
    text, n_rec = kept(eng)
    assert text == want and n_rec == want.count(b">")
    # what the records are made of, and their names
    pieces, first, ids = eng.scaffold_pieces()
    assert len(first) == n_rec + 1 and int(first[-1]) == len(pieces) and len(ids) == n_rec
    lines = want.decode("ascii").split("\n")
    assert lines[-1] == "" and len(lines) == 2 * n_rec + 1
    seqs = [seq for _, seq in case["records"]]
    n_paths = len(case["paths"])
    for r in range(n_rec):
        assert lines[2 * r] == ">" + ids[r]
        assert ids[r] == "ntJoin%d" % r if r < n_paths else ":" in ids[r]
        rec = [tuple(int(x) for x in p) for p in pieces[int(first[r]):int(first[r + 1])].tolist()]
        R.check_table([rec], [len(s) for s in seqs])
        spelled = R.spell(rec, seqs)
        assert lines[2 * r + 1] == (spelled.upper() if fold and r < n_paths else spelled), r
    # no file named: the same text; nothing written
    before = sorted(os.listdir(tmp_path))
    _, res2 = call(eng, a, case, None, keep=True, named=False, fold=fold)
    assert kept(eng)[0] == want and sorted(os.listdir(tmp_path)) == before
    assert res2["lead_strip"].tolist() == res0["lead_strip"].tolist() and res2["n_unassigned"] == res0["n_unassigned"]
    return want


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p)[:-5] for p in GOLDENS])
def test_goldens(path, tmp_path):
    case = golden_case(path)
    with MxEngine(k=15, w=10) as eng:
        a = eng.add_fasta("t", 1.0, case["fasta"])
        check_case(eng, a, case, tmp_path)
        check_case(eng, a, case, tmp_path, fold=True)


@pytest.mark.parametrize("seed", cases.FUZZ_SEEDS)
def test_fuzz_seeds(seed, tmp_path):
    case = fuzz_case(seed, tmp_path)
    with MxEngine(k=15, w=10) as eng:
        a = eng.add_fasta("t", 1.0, case["fasta"]) if seed % 5 else eng.add_records("t", 1.0, case["records"])
        check_case(eng, a, case, tmp_path)


@pytest.mark.parametrize("seed", [3, 8, 14, 21, 30])
def test_bgzf_files_and_windows_of_one_tile(seed, tmp_path, monkeypatch):
    "the kept text is the uncompressed text whatever the files are, and does not depend on the windows the files leave through"
    case = fuzz_case(seed, tmp_path)
    with MxEngine(k=15, w=10) as eng:
        a = eng.add_fasta("t", 1.0, case["fasta"])
        want = check_case(eng, a, case, tmp_path)
        plain, _ = call(eng, a, case, tmp_path / "gz_plain", keep=False, bgzf=True)
        flagged, _ = call(eng, a, case, tmp_path / "gz_keep", keep=True, bgzf=True)
        for p, q in zip(plain, flagged):
            assert read(p) == read(q), q
        assert read(flagged[0])[:2] == b"\x1f\x8b" and kept(eng)[0] == want
    monkeypatch.setenv("MXG_SCAF_WIN", "8192")   # (read once per handle)
    with MxEngine(k=15, w=10) as eng:
        a = eng.add_fasta("t", 1.0, case["fasta"])
        assert check_case(eng, a, case, tmp_path) == want
        assert "MXG_SCAF_WIN=8192" in eng.knobs()


def test_flags_that_need_a_file_and_other_refusals(tmp_path):
    case = fuzz_case(3, tmp_path)
    with MxEngine(k=15, w=10) as eng:
        a = eng.add_fasta("t", 1.0, case["fasta"])
        for kw in ({"bgzf": True}, {"fai": True}, {"report": True}):
            with pytest.raises(MxError) as err:
                call(eng, a, case, None, keep=True, named=False, **kw)
            assert err.value.code == capi.MXG_EINVAL
        with pytest.raises(ValueError):   # without the flag the assigned file has to be named, as before
            call(eng, a, case, None, keep=False, named=False)
        for fn in (eng.scaffold_text, eng.scaffold_pieces):
            with pytest.raises(MxError) as err:
                fn()
            assert err.value.code == capi.MXG_EINVAL
        call(eng, a, case, None, keep=True, named=False)
        assert kept(eng)[1] > 0
        bad = dict(case, paths=[case["paths"][0][:1]])   # a path of one node: refused, and the text of the call before is gone
        with pytest.raises(MxError) as err:
            call(eng, a, bad, None, keep=True, named=False)
        assert err.value.code == capi.MXG_EINVAL
        with pytest.raises(MxError):
            eng.scaffold_text()
        tsv = str(tmp_path / "t.tsv")
        eng.sketch(a)
        eng.write_tsv(a, tsv)
        b = eng.add_tsv("from_tsv", 1.0, tsv)
        with pytest.raises(MxError) as err:   # no text to cut from, flag or not
            call(eng, b, case, None, keep=True, named=False)
        assert err.value.code == capi.MXG_EINVAL
