"""GPU tests of the assembly report (ntjoin_amd/csrc/report.hip): mxg_assembly_report on the device-ingest and the host-ingest route
and mxg_write_scaffolds with MXG_SCAF_REPORT against the restatement of the contract (tests/_seqreport_restatement.py; no program
for this exists to compare with: QUAST and abyss-fac are absent) -- for the scaffold files, over the files as written, read back
from disk.  Every input is generated here or is a committed fixture; a 4096-byte tile is the unit that can go wrong, so the shapes
are small.  The scan over the work items has three levels (256 items a block, 256 blocks a round of the middle kernel): the third
needs more than 256 MB of text, so its width is a test knob (MXG_REPORT_SCAN_W) and test_scan_depth sets it to 4."""
import argparse
import contextlib
import gzip
import io
import os
import subprocess
import sys

import pytest

from ntjoin_amd.engine import MxEngine, MxError
from tests import _scaffold_restatement as rs, _seqreport_cases as cases, _seqreport_restatement as R
from tests._scaffold_cases import rows_of, write_fasta
from tests.conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu
EINVAL = -1
KNOBS = ("MXG_HOST_INGEST", "MXG_BGZF_PAYLOAD", "MXG_SCAF_WIN", "MXG_REPORT_SCAN_W")
FASTA = os.path.join(GOLDEN, "fasta")
SHAPES = cases.shapes()


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


def reports_of(tmp_path, texts, params=((10, 500),)):
    "every text as an assembly of handles of up to 30 -> {(name, min_gap, min_len): report}"
    out, names = {}, sorted(texts)
    for lo in range(0, len(names), 30):
        with MxEngine(k=15, w=10) as eng:
            for name in names[lo:lo + 30]:
                fa = tmp_path / (name + ".fa")
                fa.write_bytes(texts[name])
                a = eng.add_fasta(name, 1.0, str(fa))
                for mg, ml in params:
                    eng.set_report_params(mg, ml)
                    out[name, mg, ml] = R.normal(eng.assembly_report(a))
    return out


def check(got, texts, params=((10, 500),)):
    for name, text in texts.items():
        for mg, ml in params:
            assert got[name, mg, ml] == R.report(text, mg, ml), (name, mg, ml)


@pytest.mark.parametrize("route", ["device", "host"])
def test_goldens(route, env, tmp_path):
    if route == "host":
        env["MXG_HOST_INGEST"] = "1"
    texts = {name: read(os.path.join(FASTA, name)) for name in sorted(os.listdir(FASTA))}
    check(reports_of(tmp_path, texts), texts)
    want = R.report(texts["scaf.more_seqs.fa"])
    assert want["n_gaps"] > 0 and want["lower"] > 0  # (the fixtures carry what the docstrings say)
    assert R.report(texts["scaf.f-f.termN.fa"])["n"] > 0


@pytest.mark.parametrize("route", ["device", "host"])
def test_shapes(route, env, tmp_path):
    if route == "host":
        env["MXG_HOST_INGEST"] = "1"
    params = ((10, 500), (1, 0), (2, 500))
    check(reports_of(tmp_path, SHAPES, params), SHAPES, params)
    # the shapes are what their names say, at the default parameters
    gaps = lambda name: R.report(SHAPES[name])["gap_len"]  # noqa: E731
    assert gaps("run_of_min_gap_minus_1_and_min_gap") == [10]
    assert gaps("run_ends_on_last_byte_of_tile_and_next_starts_on_first") == [15, 20]
    assert gaps("two_half_runs_across_tile_border_joined") == [10] and gaps("two_half_runs_across_tile_border_base_between") == []
    assert gaps("run_cut_by_line_end_at_every_phase_crlf") == [25] * 60
    assert gaps("run_across_three_whole_tiles") == [3 * 4096 + 5, 3 * 4096 + 700]
    text = SHAPES["run_ends_on_last_byte_of_tile_and_next_starts_on_first"]
    assert text[4076:4096] == b"N" * 20 and text[4075:4076] != b"N" and text[4096:4097] != b"N"  # ends on the last byte of tile 0
    assert text[8192:8207] == b"N" * 15 and text[8191:8192] != b"N" and text[8207:8208] != b"N"  # starts on the first byte of tile 2


def test_scan_depth(env, tmp_path):
    "every level of the scan, on both routes and from a BGZF file of the same bytes"
    env["MXG_REPORT_SCAN_W"] = "4"
    text = cases.scan_depth()
    assert len(text) > 4096 * 4 * 4 * 4
    want = R.report(text)
    assert want["max_gap"] == 9000 and want["n_gaps"] > 20
    fa, gz = tmp_path / "d.fa", tmp_path / "z.fa.gz"
    fa.write_bytes(text)
    with MxEngine(k=15, w=10) as eng:
        eng.bgzf_write(text, str(gz))
        assert gzip.decompress(read(gz)) == text
        a, z = eng.add_fasta("d", 1.0, str(fa)), eng.add_fasta("z", 1.0, str(gz))
        assert R.normal(eng.assembly_report(a)) == want
        assert R.normal(eng.assembly_report(z)) == want
        assert "MXG_REPORT_SCAN_W=4" in eng.knobs()
    env["MXG_HOST_INGEST"] = "1"
    with MxEngine(k=15, w=10) as eng:
        assert R.normal(eng.assembly_report(eng.add_fasta("d", 1.0, str(fa)))) == want


# ---- MXG_SCAF_REPORT
def scaffold_files(eng, a, records, paths, out, overlap_gap, **kw):
    index = {rid: r for r, (rid, _) in enumerate(records)}
    rows, first = rows_of(paths, index)
    names = [str(out) + s for s in (".assigned.fa", ".unassigned.fa", ".bed")]
    res = eng.write_scaffolds(a, rows, first, overlap_gap=overlap_gap, assigned=names[0], unassigned=names[1], bed=names[2], **kw)
    return names, (res["lead_strip"].tolist(), res["tail_strip"].tolist(), res["n_unassigned"])


def text_of(path, bgzf):
    return gzip.decompress(read(path)) if bgzf else read(path)  # (Python's gzip reads member chains)


@pytest.mark.parametrize("win", [None, str(cases.WIN)])
@pytest.mark.parametrize("bgzf", [False, True])
@pytest.mark.parametrize("route", ["device", "host"])
def test_scaffolds(win, bgzf, route, env, tmp_path):
    records, paths, gap = cases.scaffold_case()
    want_text, leads, tails = rs.scaffolds(paths, dict(records), gap)
    # the case is what its docstring says: a header and a run of exactly min_gap N straddle window borders, strips at both ends
    assert want_text.index(">ntJoin1\n") == cases.WIN - 4
    assert want_text[2 * cases.WIN - 4:2 * cases.WIN + 6] == "N" * 10 and "N" not in want_text[2 * cases.WIN - 5] + want_text[2 * cases.WIN + 6]
    assert leads[0] == 5 and tails[1] == 10
    if win:
        env["MXG_SCAF_WIN"] = win
    if bgzf:
        env["MXG_BGZF_PAYLOAD"] = "256"
    if route == "host":
        env["MXG_HOST_INGEST"] = "1"
    fasta = str(tmp_path / "t.fa")
    write_fasta(fasta, records, 70)
    with MxEngine(k=15, w=10) as eng:
        a = eng.add_fasta("t", 1.0, fasta)
        with pytest.raises(MxError) as err:
            eng.scaffold_report("all")
        assert err.value.code == EINVAL and "MXG_SCAF_REPORT" in str(err.value)
        for fold in (False, True):
            tag = "fold" if fold else "asis"
            plain, res0 = scaffold_files(eng, a, records, paths, tmp_path / ("plain_" + tag), gap, fold_case=fold, bgzf=bgzf)
            on, res1 = scaffold_files(eng, a, records, paths, tmp_path / ("on_" + tag), gap, fold_case=fold, bgzf=bgzf, report=True)
            assert res0 == res1 and [read(n) for n in on] == [read(n) for n in plain]  # byte for byte what it is without the flag
            texts = [text_of(n, bgzf) for n in on[:2]]
            assert texts[0].decode() == rs.scaffolds(paths, dict(records), gap, fold)[0]
            for which, text in zip(("assigned", "unassigned", "all"), texts + [texts[0] + texts[1]]):
                got = R.normal(eng.scaffold_report(which))
                assert got == R.report(text), (which, fold)
            rep = eng.scaffold_report("assigned")
            assert (rep["lower"] == 0) == fold and rep["n_records"] == 3 and 12 in rep["gap_len"].tolist() and 10 in rep["gap_len"].tolist()
            assert eng.scaffold_report("unassigned")["n_records"] == res1[2] == 3
        # other parameters on the same handle: the next write reports with them
        eng.set_report_params(1, 0)
        on, _ = scaffold_files(eng, a, records, paths, tmp_path / "mg1", gap, bgzf=bgzf, report=True)
        text = text_of(on[0], bgzf) + text_of(on[1], bgzf)
        assert R.normal(eng.scaffold_report("all")) == R.report(text, 1, 0)
        if win:
            assert f"MXG_SCAF_WIN={win}" in eng.knobs()


def test_whole_scaffolder_on_the_synth_fixtures(env, tmp_path, monkeypatch):
    "Ntjoin.scaffold() with report=True: <prefix>.report.tsv, rows in order, every other file as without it"
    from ntjoin_amd.ntjoin import Ntjoin
    from ntjoin_amd.report import COLUMNS
    assert COLUMNS == R.COLUMNS
    outs = {}
    for tag, report in (("off", False), ("on", True)):
        d = tmp_path / tag
        d.mkdir()
        for fa in ("synth.ref.fa", "synth.tgt.fa"):
            os.symlink(os.path.join(FASTA, fa), d / fa)
        monkeypatch.chdir(d)
        args = argparse.Namespace(FILES=["synth.ref.fa.k32.w100.tsv"], s="synth.tgt.fa.k32.w100.tsv", l=1, p="out", k=32, n=1, t=1, overlap=True,
                                  report=report)
        nj = Ntjoin(args, fasta={"synth.ref.fa.k32.w100.tsv": "synth.ref.fa", "synth.tgt.fa.k32.w100.tsv": "synth.tgt.fa"}, w=100)
        try:
            nj.weights_list = [2]
            with contextlib.redirect_stdout(io.StringIO()):
                nj.load_minimizers_scaffold()
                files = nj.scaffold()
        finally:
            nj.close()
        outs[tag] = {n: read(d / n) for n in sorted(os.listdir(d)) if not os.path.islink(d / n)}
        assert ("report" in files) == report
    assert "out.report.tsv" not in outs["off"] and {n: v for n, v in outs["on"].items() if n != "out.report.tsv"} == outs["off"]
    base = "synth.tgt.fa.k32.w100.n1"
    parts = [outs["on"][f"{base}.{kind}.scaffolds.fa"] for kind in ("assigned", "unassigned")]
    assert parts[0].count(b">") >= 1
    want = ["\t".join(R.COLUMNS)]
    want += [R.tsv_row(fa, R.report(read(os.path.join(FASTA, fa)))) for fa in ("synth.ref.fa", "synth.tgt.fa")]
    want += [R.tsv_row(f"{base}.{kind}.scaffolds.fa", R.report(text)) for kind, text in zip(("assigned", "unassigned", "all"), parts + [parts[0] + parts[1]])]
    assert outs["on"]["out.report.tsv"].decode() == "\n".join(want) + "\n"


def test_refusals(env, tmp_path):
    "MXG_EINVAL with a message that names the cause; the handle goes on"
    fa = tmp_path / "t.fa"
    fa.write_bytes(read(os.path.join(FASTA, "scaf.f-f.fa")))
    want = R.report(read(fa))

    def refused(call, match):
        with pytest.raises(MxError) as err:
            call()
        assert err.value.code == EINVAL and match in str(err.value), str(err.value)

    with MxEngine(k=32, w=100) as eng:
        a = eng.add_fasta("t", 1.0, str(fa))
        eng.sketch(a)
        tsv = str(tmp_path / "t.tsv")
        eng.write_tsv(a, tsv)
        t = eng.add_tsv("from_tsv", 1.0, tsv)
        refused(lambda: eng.assembly_report(t), "holds no text (a minimizer table from a TSV")
        refused(lambda: eng.assembly_report(7), "no assembly 7")
        refused(lambda: eng.scaffold_report("all"), "no mxg_write_scaffolds with MXG_SCAF_REPORT")
        refused(lambda: eng.scaffold_report(3), "no file 3")
        refused(lambda: eng.set_report_params(0, 500), "min_gap is 0")
        assert R.normal(eng.assembly_report(a)) == want  # (the parameters are what they were)
        eng.set_report_params(3, 0)  # min_len = 0 is allowed
        assert R.normal(eng.assembly_report(a)) == R.report(read(fa), 3, 0)
    with MxEngine(k=32, w=100, drop_seq=True) as eng:
        refused(lambda: eng.assembly_report(eng.add_fasta("t", 1.0, str(fa))), "text dropped by MXG_FLAG_DROP_SEQ")
    assert sorted(os.listdir(tmp_path)) == ["t.fa", "t.tsv"]  # nothing else was written


# ---- the command line: every run a child process under a time limit of its own
ENV = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
LIMIT = ["timeout", "-k", "10", "120"]
OUT = "scaf.f-f.termN.fa.k32.w1000.n1"
ASSEMBLE = [sys.executable, "-m", "ntjoin_amd.assemble", "-p", "run", "-n", "1", "-s", "scaf.f-f.termN.fa.k32.w1000.tsv", "-l", "1", "-r", "2", "-k", "32",
            "ref.fa.k32.w1000.tsv"]
MAKE = ["make", "-f", os.path.join(REPO, "ntJoin-mx"), "scaffold", "target=scaf.f-f.termN.fa", "references=ref.fa", "reference_weights=2", "k=32", "w=1000",
        "n=1", "prefix=run", "overlap=False"]


def child(cwd, words):
    res = subprocess.run(LIMIT + words, cwd=cwd, env=ENV, capture_output=True, text=True, check=False)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    return res


def fresh(tmp_path, name):
    d = tmp_path / name
    d.mkdir()
    for fa in ("scaf.f-f.termN.fa", "ref.fa"):
        os.symlink(os.path.join(FASTA, fa), d / fa)
    return d


def files(d):
    return {n: read(d / n) for n in sorted(os.listdir(d)) if not os.path.islink(d / n)}


def check_tsv(got, names_texts, mg=10, ml=500):
    want = ["\t".join(R.COLUMNS)] + [R.tsv_row(name, R.report(text, mg, ml)) for name, text in names_texts]
    assert got.decode() == "\n".join(want) + "\n"


def test_assemble_report(env, tmp_path):
    off, on = fresh(tmp_path, "off"), fresh(tmp_path, "on")
    child(off, ASSEMBLE)
    child(on, ASSEMBLE + ["--report", "--report_min_gap", "2", "--report_min_len", "0"])
    before, after = files(off), files(on)
    assert "run.report.tsv" not in before and {n: v for n, v in after.items() if n != "run.report.tsv"} == before
    parts = [after[f"{OUT}.{kind}.scaffolds.fa"] for kind in ("assigned", "unassigned")]
    rows = [(fa, read(os.path.join(FASTA, fa))) for fa in ("ref.fa", "scaf.f-f.termN.fa")]
    rows += [(f"{OUT}.{kind}.scaffolds.fa", text) for kind, text in zip(("assigned", "unassigned", "all"), parts + [parts[0] + parts[1]])]
    check_tsv(after["run.report.tsv"], rows, 2, 0)
    # a reference loaded from its TSV (the first run left it): one line on stderr, no row
    res = child(on, ASSEMBLE + ["--report"])
    assert "ref.fa.k32.w1000.tsv was loaded from its TSV: the report has no row for it" in res.stderr
    check_tsv(read(on / "run.report.tsv"), rows[1:])


def test_make_scaffold_report(env, tmp_path):
    d = fresh(tmp_path, "run")
    child(d, MAKE + ["report=True", "gz=True"])
    after = files(d)
    rows = [(fa, read(os.path.join(FASTA, fa))) for fa in ("ref.fa", "scaf.f-f.termN.fa")]
    rows += [(f"{OUT}.{kind}.scaffolds.fa.gz", gzip.decompress(after[f"{OUT}.{kind}.scaffolds.fa.gz"])) for kind in ("assigned", "unassigned", "all")]
    check_tsv(after["run.report.tsv"], rows)
