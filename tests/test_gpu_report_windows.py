"""GPU tests of the report's window route (ntjoin_amd/csrc/report.hip, source RS_WINDOW): mxg_write_scaffolds with MXG_SCAF_REPORT
reports on both scaffold FASTAs window by window as they leave.  What runs on this route only: the per-lane masks made from the
piece table (rep_fetch), the state the device keeps between two windows (k_rep_tile_scan), the gap and contig lists that grow from
window to window and keep what they hold (rep_grow in rep_pass), and the plain tiles that pass 2 does not read (k_rep_emit).

The expectation is always the restatement (tests/_seqreport_restatement.py) over the files as written, read back from disk, and every
call with the flag must leave byte for byte the files of the same call without it.

 1. the placed shapes of tests/_seqreport_cases.py window_shapes(): borders at every lane phase, several in a lane, headers across
    lane, wave, tile and window borders and longer than a tile, runs made of pieces, runs and contigs across whole windows, lists that
    grow, empty files, case folding -- at the default window and at one emit tile a window, on both ingest routes, plain and BGZF;
 2. the lists' growth witnessed on the line "[mxg] report items=... run_starts=..." that MXG_DEBUG_IO=1 prints per pass;
 3. every seed of the scaffold fuzz and every golden of tests/golden/scaffolds through the report;
 4. all three levels of the scan (MXG_REPORT_SCAN_W=4) in one pass and in many passes of two tiles;
 5. a tile of line ends inside an N run (mxg_assembly_report on the device-ingest route): the one way a tile without bases is entered
    with an open run -- on the window route such a tile lies inside a header, behind its border."""
import glob
import gzip
import os
import re

import pytest

from ntjoin_amd.engine import MxEngine
from tests import _oracle, _scaffold_cases as scaf, _seqreport_cases as cases, _seqreport_restatement as R

pytestmark = pytest.mark.gpu
KNOBS = ("MXG_HOST_INGEST", "MXG_BGZF_PAYLOAD", "MXG_SCAF_WIN", "MXG_REPORT_SCAN_W", "MXG_DEBUG_IO")
PARAMS = ((10, 500), (1, 0), (2, 500))
WHICH = ("assigned", "unassigned", "all")
WITNESS = re.compile(r"\[mxg\] report items=(\d+) pass1_ms=[0-9.]+ scan_ms=[0-9.]+ pass2_ms=[0-9.]+ run_starts=(\d+)\n")
SHAPES = cases.window_shapes()  # (made once, never changed)
# (window, ingest route, BGZF): every shape at both window sizes, on both routes, plain and compressed
CONFIGS = [(None, "device", False), (str(cases.WIN), "device", False), (str(cases.WIN), "host", True), (None, "host", False),
           (str(cases.WIN), "device", True)]
GOLDENS = sorted(glob.glob(os.path.join(scaf.GOLDEN, "scaffolds", "*.json")))


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


def set_knobs(env, win=None, route="device", bgzf=False):
    "(the handle reads them when it is made)"
    for name, value in (("MXG_SCAF_WIN", win), ("MXG_HOST_INGEST", "1" if route == "host" else None), ("MXG_BGZF_PAYLOAD", "256" if bgzf else None)):
        if value is None:
            env.pop(name, None)
        else:
            env[name] = value


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


def text_of(path, bgzf):
    return gzip.decompress(read(path)) if bgzf else read(path)  # (Python's gzip reads member chains)


def scaffold_files(eng, a, records, paths, out, overlap_gap, **kw):
    index = {rid: r for r, (rid, _) in enumerate(records)}
    rows, first = scaf.rows_of(paths, index)
    names = [str(out) + s for s in (".assigned.fa", ".unassigned.fa", ".bed")]
    res = eng.write_scaffolds(a, rows, first, overlap_gap=overlap_gap, assigned=names[0], unassigned=names[1], bed=names[2], **kw)
    return names, (res["lead_strip"].tolist(), res["tail_strip"].tolist(), res["n_unassigned"])


def reported(eng, a, case, out, fold=False, bgzf=False, params=((10, 500),)):
    """one call without the flag, then one with it per pair of parameters: the files byte for byte those of the first call, the three
    reports those of the restatement over the files -> the two FASTA texts"""
    records, paths, gap = case
    plain, res0 = scaffold_files(eng, a, records, paths, str(out) + "_plain", gap, fold_case=fold, bgzf=bgzf)
    texts = None
    for mg, ml in params:
        eng.set_report_params(mg, ml)
        on, res1 = scaffold_files(eng, a, records, paths, f"{out}_on_{mg}_{ml}", gap, fold_case=fold, bgzf=bgzf, report=True)
        assert res0 == res1 and [read(n) for n in on] == [read(n) for n in plain]
        texts = [text_of(n, bgzf) for n in on[:2]]
        for which, text in zip(WHICH, texts + [texts[0] + texts[1]]):
            assert R.normal(eng.scaffold_report(which)) == R.report(text, mg, ml), (which, mg, ml)
    return texts


# ---- 1. the placed shapes
@pytest.mark.parametrize("win,route,bgzf", CONFIGS, ids=[f"win{w or 'default'}-{r}-{'bgzf' if b else 'plain'}" for w, r, b in CONFIGS])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes(name, win, route, bgzf, env, tmp_path):
    """(header_longer_than_a_tile: the library takes an id of 2 x 4096 + 50 bytes as it is; no shorter one is used)"""
    set_knobs(env, win, route, bgzf)
    case = SHAPES[name]
    fasta = str(tmp_path / "t.fa")
    scaf.write_fasta(fasta, case[0], 70)
    with MxEngine(k=15, w=10) as eng:
        a = eng.add_fasta("t", 1.0, fasta)
        for fold in (False, True) if name in cases.FOLD_TOO else (False,):
            texts = reported(eng, a, case, tmp_path / f"fold{int(fold)}", fold, bgzf, PARAMS)
            assert tuple(texts) == cases.window_texts(case, fold)  # the offsets the builder asserted are those of the files
            if name in cases.FOLD_TOO:
                rep = eng.scaffold_report("assigned")
                assert (rep["lower"] == 0) == fold and rep["other"] > 0 and rep["t"] > 0
                assert eng.scaffold_report("unassigned")["lower"] > 0  # (the unassigned file is never folded)
        if name.startswith("empty_files"):
            rep = R.normal(eng.scaffold_report("unassigned"))
            assert texts[1] == b"" and rep == R.report(b"", *PARAMS[-1])
            assert rep["n_records"] == rep["bases"] == rep["n_gaps"] == rep["contig"]["n"] == 0 and rep["gap_len"] == rep["contig_len"] == []
        if win:
            assert f"MXG_SCAF_WIN={win}" in eng.knobs()


# ---- 2. the lists grow and keep what they hold
def test_lists_grow_and_keep(env, capfd, tmp_path):
    """six windows with 1, 3, 9, 27, 81 and 243 runs on a fresh handle: the witness line of every pass names the runs begun so far, the
    lists are made for that many plus two and half as many again, so a pass whose figure is more than 1.5 times the one before finds
    them too small, and the entries of the windows before must come along"""
    set_knobs(env, str(cases.WIN))
    env["MXG_DEBUG_IO"] = "1"
    case = SHAPES["lists_grow_three_times"]
    want = cases.window_texts(case)
    fasta = str(tmp_path / "t.fa")
    scaf.write_fasta(fasta, case[0], 70)
    with MxEngine(k=15, w=10) as eng:
        a = eng.add_fasta("t", 1.0, fasta)
        capfd.readouterr()
        on, _ = scaffold_files(eng, a, *case[:2], tmp_path / "on", case[2], report=True)
        lines = [(int(items), int(starts)) for items, starts in WITNESS.findall(capfd.readouterr().err)]
        rep = R.normal(eng.scaffold_report("assigned"))
    assert (read(on[0]), read(on[1])) == want
    windows = [-(-len(text) // cases.WIN) for text in want]
    assert windows[0] == len(cases.GROWTH) + 1 and len(lines) == sum(windows), lines  # one pass per window of either file
    assert [items for items, _ in lines] == [2] * len(cases.GROWTH) + [1, 1]
    starts = [s for _, s in lines[:windows[0]]]
    print("run_starts per window:", starts)
    grows = [starts[i] + 2 > 1.5 * (starts[i - 1] + 2) for i in range(1, len(starts))]
    assert any(all(grows[i:i + 3]) for i in range(len(grows) - 2)), starts
    assert starts[-1] >= sum(cases.GROWTH)
    expect = R.report(want[0])
    assert rep["gap_len"] == expect["gap_len"] and len(rep["gap_len"]) == sum(cases.GROWTH) and rep["contig_len"] == expect["contig_len"]


# ---- 3. the scaffold stage's fuzz and goldens
SCAF_CASES = [("fuzz", s) for s in scaf.FUZZ_SEEDS] + [("golden", g) for g in GOLDENS]
SCAF_IDS = [f"fuzz{s}" for s in scaf.FUZZ_SEEDS] + [os.path.basename(g)[:-5] for g in GOLDENS]


@pytest.mark.parametrize("kind,which", SCAF_CASES, ids=SCAF_IDS)
def test_fuzz_and_goldens(kind, which, env, tmp_path):
    "pieces that begin and end inside N runs, N runs longer than an emit tile, strips, cut nodes and records that are N throughout"
    if kind == "fuzz":
        case = scaf.fuzz_case(which)
        fasta = str(tmp_path / "t.fa")
        scaf.write_fasta(fasta, case["records"], case["width"], case["final_newline"])
        records, paths, gap, fold, bgzf, kw = case["records"], case["paths"], case["overlap_gap"], case["fold"], which % 2 == 1, (15, 10)
    else:
        doc, fasta = scaf.load_golden(which)
        records, paths, gap = _oracle.read_fasta(fasta), scaf.golden_nodes(doc), doc["meta"]["overlap_gap"] if doc["meta"]["overlap"] else None
        fold, bgzf, kw = False, False, (32, 100)
    got = []
    for win in (str(cases.WIN), None):
        set_knobs(env, win)
        with MxEngine(k=kw[0], w=kw[1]) as eng:
            a = eng.add_fasta("t", 1.0, fasta)
            got.append(reported(eng, a, (records, paths, gap), tmp_path / f"win{win}", fold, bgzf))
    assert got[0] == got[1] and len(got[0][0]) > 0


# ---- 4. the scan's three levels
def test_scan_depth(env, tmp_path):
    "more than 4 x 4 x 4 items in one pass at the default window, and 41 passes of two items at one emit tile a window"
    env["MXG_REPORT_SCAN_W"] = "4"
    case = cases.window_scan_depth()
    want = cases.window_texts(case)
    assert len(want[0]) > 4096 * 4 * 4 * 4
    expect = R.report(want[0])
    assert expect["max_gap"] == 9000 and 5000 in expect["gap_len"] and expect["n_gaps"] > 20
    fasta = str(tmp_path / "t.fa")
    scaf.write_fasta(fasta, case[0], 70)
    for win in (None, str(cases.WIN)):
        set_knobs(env, win)
        with MxEngine(k=15, w=10) as eng:
            a = eng.add_fasta("t", 1.0, fasta)
            assert tuple(reported(eng, a, case, tmp_path / f"win{win}")) == want
            assert "MXG_REPORT_SCAN_W=4" in eng.knobs() and (win is None or f"MXG_SCAF_WIN={win}" in eng.knobs())


# ---- 5. a tile without a base, entered with an open run
def test_tile_of_line_ends_inside_a_run(env, tmp_path):
    text = cases.line_end_tile()
    want = R.report(text)
    assert want["gap_len"] == [25] and want["contig_len"] == [50, 100]
    fa = tmp_path / "t.fa"
    fa.write_bytes(text)
    with MxEngine(k=15, w=10) as eng:
        assert R.normal(eng.assembly_report(eng.add_fasta("t", 1.0, str(fa)))) == want
