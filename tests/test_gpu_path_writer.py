"""GPU tests of the .path / AGP writer (mxg_write_paths, csrc/pathtext.hip; reference print_scaffolds :605-610, write_agp :346-376,
write_agp_unassigned :379-404): the goldens, paths that span lanes, waves and blocks, every digit border, orientations, cuts and
strips, small output windows, either file into a FIFO, the unassigned lines, every refusal, one larger call, and the routing inside Ntjoin.print_scaffolds.
The writer never reads the bases, so the assemblies are a handful of short records.  Every comparison is byte for byte against
the restatement (tests/_path_text_restatement.py) or, for the generated families of tests/golden/scaffolds/families, against the text
the reference itself wrote."""
import argparse
import glob
import os
import random
import time

import numpy as np
import pytest

from ntjoin_amd.engine import MxEngine, MxError
from ntjoin_amd.ntjoin import Ntjoin
from tests import _fifo, _oracle, _path_text_restatement as pt, _scaffold_cases as cases, _scaffold_pin as pin, _scaffold_restatement as rs

pytestmark = pytest.mark.gpu

CASES = sorted(glob.glob(os.path.join(cases.GOLDEN, "scaffolds", "*.json")))
IDS = [os.path.basename(c)[:-5] for c in CASES]
EINVAL, ELIMIT = -1, -5
# ids of 1, 2, 31, 32, 33 and 300 bytes; some look like the fields behind them
RECORDS = [("a", "ACGTACGTAC"), ("b+", "ACGTACGTAC"), ("c" * 27 + "+:1-", "ACGTACGTAC"), ("d" * 32, "ACGTACGTAC"), ("e-:7-9" + "e" * 27, "ACGTACGTAC"),
           ("f" * 300, "ACGTACGTAC")]
assert [len(r[0]) for r in RECORDS] == [1, 2, 31, 32, 33, 300]
NAMES = [r[0] for r in RECORDS]
MAX = 4294967295


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


@pytest.fixture(scope="module")
def eng():
    with MxEngine(k=4, w=2) as e:
        e.add_records("t", 1.0, RECORDS)
        yield e


def write(eng, a, paths, leads, tails, out, index, agp=True, unassigned=False, first_line="t.fa"):
    "one call of the library -> (.path bytes, AGP bytes or None)"
    rows, first = cases.rows_of(paths, index)
    names = [str(out) + ".path", str(out) + ".agp"]
    eng.write_paths(a, rows, first, lead_strip=leads, tail_strip=tails, first_line=first_line, path=names[0], agp=names[1] if agp else None,
                    agp_unassigned=unassigned)
    assert agp or not os.path.exists(names[1])
    return read(names[0]), read(names[1]) if agp else None


def check(eng, paths, leads, tails, out):
    index = {rid: r for r, rid in enumerate(NAMES)}
    text, agp = pt.by_regex(paths, leads, tails, "t.fa")
    got = write(eng, 0, paths, leads, tails, out, index)
    assert got[0] == text.encode("ascii")
    assert got[1] == agp.encode("ascii")
    return got


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_goldens(case, tmp_path):
    "the golden's nodes, cuts and strips through write_paths, with and without the AGP: the reference's own .path text"
    doc, fasta = cases.load_golden(case)
    records = _oracle.read_fasta(fasta)
    paths = cases.golden_nodes(doc)
    _text, leads, tails = rs.scaffolds(paths, dict(records), doc["meta"]["overlap_gap"] if doc["meta"]["overlap"] else None)
    index = {rid: r for r, (rid, _) in enumerate(records)}
    text, agp = pt.by_regex(paths, leads, tails, doc["meta"]["fasta"])
    with MxEngine(k=4, w=2) as e:
        a = e.add_records("t", 1.0, [(rid, "ACGT") for rid, _ in records])
        got = write(e, a, paths, leads, tails, tmp_path / "with", index, first_line=doc["meta"]["fasta"])
        assert got[0] == doc["path"].encode("ascii") == text.encode("ascii") and got[1] == agp.encode("ascii")
        assert write(e, a, paths, leads, tails, tmp_path / "without", index, agp=False, first_line=doc["meta"]["fasta"])[0] == got[0]


def node(rng, gap=None):
    start = rng.choice([0, 1, 7, 1000, 123456])
    return (rng.choice(NAMES), rng.choice("+-"), start, start + rng.randint(1, 5000), rng.choice([0, 1, 20, 137]) if gap is None else gap, 0, 0)


def test_paths_across_lanes_waves_and_blocks(eng, tmp_path):
    "`at` is a sum segmented by path: paths of every length around 64, 256 and 1024 nodes, two-node paths between them, both orders"
    rng = random.Random(5)
    paths = []
    for m in (2, 3, 63, 64, 65, 255, 256, 257, 1024, 1025, 5000):
        paths.append([node(rng) for _ in range(m)])
        paths.append([node(rng), node(rng)])
    for order in (paths, paths[::-1]):
        zeros = [0] * len(order)
        got = check(eng, order, zeros, zeros, tmp_path / "o")
        assert got[1].count(b"\n") == 2 * sum(len(p) for p in order) - len(order)


def test_digit_borders(eng, tmp_path):
    """coordinates, gaps and running sums on either side of 10, 100, ..., 10^9 and at 2^32 - 1; `at` beyond 2^32 in the middle of a line;
    path numbers across ntJoin9 / ntJoin10 and ntJoin999 / ntJoin1000; a gap of 0 in the middle; a gap of 2^32 - 1"""
    borders = sorted({10 ** d - 1 for d in range(1, 10)} | {10 ** d for d in range(1, 10)} | {MAX})
    paths = []
    for i, v in enumerate(borders):
        for n in (v - 1, v):
            start = min(v, MAX - 5)
            # end = n and the sum at + n - 1 = n at the border, the gap and the next `at` behind it, a start at the border
            paths.append([(NAMES[i % 6], "+", 0, n, v, 0, 0), (NAMES[(i + 1) % 6], "-", start, start + 5, v - 1, 0, 0), (NAMES[(i + 2) % 6], "+", v - 1, v, 0, 0, 0)])
    big = 4000000000
    paths.append([("a", "+", 0, big, 0, 0, 0), ("b+", "-", 5, big + 5, MAX, 0, 0), ("a", "+", 0, big, 7, 0, 0), ("a", "-", 0, big, 0, 0, 0)])
    rng = random.Random(9)
    while len(paths) < 1003:
        paths.append([node(rng), node(rng)])
    zeros = [0] * len(paths)
    text, agp = check(eng, paths, zeros, zeros, tmp_path / "o")
    for name in (b"ntJoin9\t", b"ntJoin10\t", b"ntJoin999\t", b"ntJoin1000\t", b"ntJoin1002\t"):
        assert b"\n" + name in text and b"\n" + name in agp
    p = len(borders) * 2
    assert f"ntJoin{p}\t{big + 1}\t{big}\t2\tN\t0\tscaffold".encode() in agp                      # the gap of 0
    assert f"ntJoin{p}\t{2 * big + 1}\t{2 * big + MAX}\t4\tN\t{MAX}\tscaffold".encode() in agp   # the gap of 2^32 - 1
    assert f"ntJoin{p}\t{3 * big + MAX + 8}\t{4 * big + MAX + 7}\t7\tW\ta\t1\t{big}\t-".encode() in agp
    assert b"\t12000000000\t" in write(eng, 0, [[("a", "+", 0, big, 0, 0, 0)] * 3], [0], [0], tmp_path / "s", {"a": 0})[1]


def cut_and_strip_paths():
    "'+' and '-' with all four combinations of cuts as first, middle and last node; strips on '+' and '-' end nodes; both strips on two nodes"
    paths, leads, tails = [], [], []
    for ori in "+-":
        for sa, ea in ((0, 0), (3, 0), (0, 70), (3, 70)):
            for lead, tail in ((0, 0), (2, 5)):
                paths.append([("a", ori, 100, 200, 20, sa, ea), ("b+", ori, 1000, 1100, 0, sa, ea), ("d" * 32, ori, 50, 150, 9, sa, ea)])
                leads.append(lead)
                tails.append(tail)
    for o1 in "+-":
        for o2 in "+-":
            paths.append([("f" * 300, o1, 10, 90, 1, 0, 0), ("a", o2, 10, 90, 0, 0, 0)])
            leads.append(11)
            tails.append(13)
    return paths, leads, tails


def test_orientations_cuts_and_strips(eng, tmp_path):
    paths, leads, tails = cut_and_strip_paths()
    text, _agp = check(eng, paths, leads, tails, tmp_path / "o")
    assert pt.direct(paths, leads, tails, "t.fa")[0].encode("ascii") == text
    lines = text.decode("ascii").splitlines()
    # a strip and a cut on one end node: the coordinates the host loop gave (Ntjoin._path_coords on the stripped interval)
    assert lines[8] == "ntJoin7\ta+:105-172 20N b++:1003-1070 0N " + "d" * 32 + "+:53-120"
    assert lines[16] == "ntJoin15\ta-:128-195 20N b+-:1030-1097 0N " + "d" * 32 + "-:80-147"
    assert lines[-1] == "ntJoin19\t" + "f" * 300 + "-:10-79 1N a-:23-90"


@pytest.mark.parametrize("win", ["1", "7", "64", "4093"])
def test_small_windows_equal_the_default(win, tmp_path, monkeypatch):
    "MXG_PATH_WIN: bytes of text per device window, parsed once per handle; either file in many windows"
    paths, leads, tails = cut_and_strip_paths()
    rng = random.Random(3)
    paths.append([node(rng) for _ in range(300)])
    leads.append(0)
    tails.append(0)
    index = {rid: r for r, rid in enumerate(NAMES)}
    text, agp = pt.by_regex(paths, leads, tails, "t.fa")
    assert len(text) > 2 * 4093 and len(agp) > 2 * 4093
    if win == "1":  # (one launch per byte: a shorter input)
        paths, leads, tails = paths[:8], leads[:8], tails[:8]
        text, agp = pt.by_regex(paths, leads, tails, "t.fa")
    monkeypatch.setenv("MXG_PATH_WIN", win)
    with MxEngine(k=4, w=2) as e:
        a = e.add_records("t", 1.0, RECORDS)
        got = write(e, a, paths, leads, tails, tmp_path / "o", index)
        assert f"MXG_PATH_WIN={win}" in e.knobs()
    assert got == (text.encode("ascii"), agp.encode("ascii"))


@pytest.mark.parametrize("which", [0, 1], ids=["path", "agp"])
def test_a_fifo_takes_the_windows_in_order(which, tmp_path, monkeypatch):
    """either file into a FIFO (no offsets: the first line and the windows are written in order at the descriptor's own position),
    in windows of 7 bytes: the bytes of the same call into a regular file"""
    paths, leads, tails = cut_and_strip_paths()
    paths, leads, tails = paths[:4] + paths[-4:], leads[:4] + leads[-4:], tails[:4] + tails[-4:]  # (ids of 1 to 300 bytes)
    index = {rid: r for r, rid in enumerate(NAMES)}
    rows, first = cases.rows_of(paths, index)
    text, agp = pt.by_regex(paths, leads, tails, "t.fa")
    monkeypatch.setenv("MXG_PATH_WIN", "7")
    with MxEngine(k=4, w=2) as e:
        a = e.add_records("t", 1.0, RECORDS)
        want = write(e, a, paths, leads, tails, tmp_path / "o", index)
        assert want == (text.encode("ascii"), agp.encode("ascii")) and "MXG_PATH_WIN=7" in e.knobs()
        assert all(3 * 7 < len(w) < 4096 for w in want)  # three windows or more; far below any pipe's capacity
        names = [str(tmp_path / "f.path"), str(tmp_path / "f.agp")]
        with _fifo.fifo_reader(names[which], len(want[which])) as drain:
            e.write_paths(a, rows, first, lead_strip=leads, tail_strip=tails, first_line="t.fa", path=names[0], agp=names[1])
            assert drain() == want[which]
        assert read(names[1 - which]) == want[1 - which]


def test_unassigned_lines_follow_the_last_path(tmp_path):
    "the intervals and strips of a real write_scaffolds: N-only and N-flanked leftovers, as Ntjoin._write_agp_unassigned writes them"
    records = [("one", "NNACGTACGTNN" + "ACGT" * 5), ("two", "ACGTACGTAC" + "NNNN" + "nnACGTn" + "ACGTACGT"), ("allN", "NNNNnnNN"), ("free", "nACGTACGTAN")]
    paths = [[("one", "+", 12, 32, 5, 0, 0), ("two", "-", 0, 10, 0, 0, 0)], [("two", "+", 21, 29, 0, 0, 0), ("one", "-", 2, 10, 0, 0, 0)]]
    index = {rid: r for r, (rid, _) in enumerate(records)}
    rows, first = cases.rows_of(paths, index)
    names = [str(tmp_path / f) for f in ("x.fa", "x.un.fa", "x.bed", "x.path", "x.agp", "host.agp")]
    with MxEngine(k=4, w=2) as e:
        a = e.add_records("t", 1.0, records)
        with pytest.raises(MxError, match="MXG_PATHS_AGP_UNASSIGNED needs") as ei:  # no write_scaffolds yet
            e.write_paths(a, rows, first, first_line="t.fa", path=names[3], agp=names[4], agp_unassigned=True)
        assert ei.value.code == EINVAL and not os.path.exists(names[3]) and not os.path.exists(names[4])
        res = e.write_scaffolds(a, rows, first, assigned=names[0], unassigned=names[1], bed=names[2])
        e.write_paths(a, rows, first, lead_strip=res["lead_strip"], tail_strip=res["tail_strip"], first_line="t.fa", path=names[3], agp=names[4],
                      agp_unassigned=True)
        host = Ntjoin.__new__(Ntjoin)
        host._engine = e
        with open(names[5], "w", encoding="utf-8") as fh:
            host._write_agp_unassigned(fh, names[2])
        # with no path at all the AGP holds the unassigned lines alone, the .path file its first line
        e.write_paths(a, [], [0], first_line="t.fa", path=names[3] + "0", agp=names[4] + "0", agp_unassigned=True)
    text, agp = pt.by_regex(paths, res["lead_strip"].tolist(), res["tail_strip"].tolist(), "t.fa")
    tail = read(names[5])
    # (one:0-2, one:10-12 and allN:0-8 are N throughout: in the BED only)
    assert tail == b"two:10-21\t1\t4\t1\tW\ttwo\t17\t20\t+\nfree:0-11\t1\t9\t1\tW\tfree\t2\t10\t+\n"
    assert read(names[2]).count(b"\n") == 5
    assert read(names[3]) == text.encode("ascii") and read(names[4]) == agp.encode("ascii") + tail
    assert read(names[3] + "0") == b"t.fa\n" and read(names[4] + "0") == tail


def test_refusals_write_nothing(eng, tmp_path):
    "every MXG_EINVAL / MXG_ELIMIT of the contract: its code, its message, and no file; then the one valid empty call"
    good = [(0, 0, 12, 5, 0, 0, 0), (1, 0, 10, 0, 0, 0, 1)]
    names = [str(tmp_path / "x.path"), str(tmp_path / "x.agp")]

    def fails(code, match, rows, pf, lead=None, tail=None):
        with pytest.raises(MxError, match=match) as ei:
            eng.write_paths(0, rows, pf, lead_strip=lead, tail_strip=tail, first_line="t.fa", path=names[0], agp=names[1])
        assert ei.value.code == code
        assert not any(os.path.exists(f) for f in names)

    fails(EINVAL, "path 1 has 1 node", good + [good[0]], [0, 2, 3])
    fails(EINVAL, "path 0 has 0 node", good, [0, 0, 2])
    fails(EINVAL, r"path 0 node 1: \[4, 4\) is not a segment", [good[0], (1, 4, 4, 0, 0, 0, 0)], [0, 2])
    fails(EINVAL, r"path 1 node 0: \[9, 4\) is not a segment", good + [(1, 9, 4, 0, 0, 0, 0), good[1]], [0, 2, 4])
    fails(EINVAL, "path 0 node 0: end_adjust 13", [(0, 0, 12, 5, 0, 13, 0), good[1]], [0, 2])
    fails(EINVAL, "path 0 node 1: no record 6", [good[0], (6, 0, 1, 0, 0, 0, 0)], [0, 2])
    fails(EINVAL, r"path_first\[0\] is 1", good + good, [1, 4])
    fails(EINVAL, "path_first is not increasing at path 0", good + good, [0, 4, 2])
    # an adjusted interval that is empty or inverted: by the cuts, and only by the strips; the lowest node is named
    many = good * 700
    fails(EINVAL, "path 650 node 1: the adjusted interval is empty or inverted", many[:1301] + [(1, 0, 10, 0, 7, 3, 1)] + many[1302:-2] + [(0, 0, 12, 5, 9, 9, 0), good[1]],
          list(range(0, 1401, 2)))
    fails(EINVAL, "path 0 node 0: the adjusted interval is empty or inverted", good, [0, 2], lead=[12], tail=[0])
    fails(EINVAL, "path 0 node 1: the adjusted interval is empty or inverted", good, [0, 2], lead=[0], tail=[10])
    node = np.zeros(2, dtype=MxEngine.SCAFFOLD_NODE)
    pf = np.array([0, 1 << 31], dtype=np.uint64)
    rc = eng._lib.mxg_write_paths(eng._h, 0, node.ctypes.data, pf.ctypes.data, 1, None, None, b"t.fa", names[0].encode(), names[1].encode(), 0)
    assert rc == ELIMIT and not any(os.path.exists(f) for f in names)
    pf = np.array([0, 2], dtype=np.uint64)
    rc = eng._lib.mxg_write_paths(eng._h, 0, node.ctypes.data, pf.ctypes.data, 1, None, None, b"t.fa", None, names[1].encode(), 0)
    assert rc == EINVAL and not any(os.path.exists(f) for f in names)
    with pytest.raises(MxError, match="no assembly 3"):
        eng.write_paths(3, good, [0, 2], first_line="t.fa", path=names[0])
    # no path at all: the first line, and an empty AGP
    eng.write_paths(0, [], [0], first_line="some name.fa", path=names[0], agp=names[1])
    assert read(names[0]) == b"some name.fa\n" and read(names[1]) == b""
    # ... and the handle still writes
    eng.write_paths(0, good, [0, 2], first_line="t.fa", path=names[0])
    assert read(names[0]) == b"t.fa\nntJoin0\ta+:0-12 5N b+-:0-10\n"


def test_one_larger_call(eng, tmp_path, capsys):
    "10^4 paths of 10 nodes; the device call's and the host loop's wall time are printed, none is asserted"
    rng = random.Random(11)
    paths = [[node(rng) for _ in range(10)] for _ in range(10000)]
    for path in paths:
        path[-1] = path[-1][:4] + (0,) + path[-1][5:]
    zeros = [0] * len(paths)
    index = {rid: r for r, rid in enumerate(NAMES)}
    rows, first = cases.rows_of(paths, index)
    arr = np.array(rows, dtype=np.int64)
    nodes = np.zeros(len(arr), dtype=MxEngine.SCAFFOLD_NODE)
    for j, col in enumerate(("record", "start", "end", "gap_size", "start_adjust", "end_adjust", "reverse")):
        nodes[col] = arr[:, j]
    names = [str(tmp_path / f) for f in ("d.path", "d.agp", "h.path", "h.agp", "h.bed")]
    eng.write_paths(0, nodes, first, first_line="t.fa", path=names[0], agp=names[1])  # (the windows and the pinned pool exist from here on)
    t0 = time.perf_counter()
    eng.write_paths(0, nodes, first, first_line="t.fa", path=names[0], agp=names[1])
    t_dev = time.perf_counter() - t0
    host = Ntjoin.__new__(Ntjoin)
    host._engine = eng
    open(names[4], "w", encoding="ascii").close()
    kept = [([[c, o, s, e, 0, 0, 0, g, g] for c, o, s, e, g, _sa, _ea in path], [(0, 0)] * len(path)) for path in paths]
    t0 = time.perf_counter()
    host._write_path_host({"path": names[2], "agp": names[3], "bed": names[4]}, "t.fa", kept, zeros, zeros)
    t_host = time.perf_counter() - t0
    with capsys.disabled():
        print(f"\n[path writer] 10^5 nodes, {os.path.getsize(names[0]) + os.path.getsize(names[1])} bytes: mxg_write_paths {t_dev * 1e3:.1f} ms, "
              f"_write_path_host {t_host * 1e3:.1f} ms")
    assert read(names[0]) == read(names[2]) and read(names[1]) == read(names[3])
    assert read(names[0]).count(b"\n") == 10001 and read(names[1]).count(b"\n") == 190000
    text, agp = pt.by_regex(paths[:50], zeros[:50], zeros[:50], "t.fa")
    assert read(names[0]).startswith(text.encode("ascii")) and read(names[1]).startswith(agp.encode("ascii"))


def test_print_scaffolds_takes_the_host_route_only_for_refused_intervals(tmp_path, monkeypatch):
    doc, fasta = cases.load_golden(os.path.join(cases.GOLDEN, "scaffolds", "f-f.json"))
    name = doc["meta"]["fasta"]
    monkeypatch.chdir(tmp_path)
    os.symlink(fasta, name)
    os.symlink(os.path.join(cases.GOLDEN, "fasta", "ref.fa"), "ref.fa")
    args = argparse.Namespace(k=32, FILES=["ref.fa.k32.w1000.tsv"], s=name + ".k32.w1000.tsv", l=1.0, p="out", n=1)

    class HostRoute(Exception):
        pass

    def refuse(*_a, **_k):
        raise HostRoute()

    nj = Ntjoin(args, fasta={args.FILES[0]: "ref.fa", args.s: name}, w=1000)
    try:
        nj.weights_list = [2.0]
        nj.load_minimizers_scaffold()
        host = nj._write_path_host
        monkeypatch.setattr(nj, "_write_path_host", refuse)
        files = nj.print_scaffolds(doc["paths"], None, n=1, agp=True)
        assert read(files["path"]) == doc["path"].encode("ascii")
        # a middle node whose cuts invert its interval (it gives the scaffold no text, which the scaffold stage accepts)
        one, two = doc["paths"][0]
        paths = [[one, two[:2] + [0, 100] + two[4:7] + [20, 20], two[:2] + [100, two[3]] + two[4:]]]
        cuts = [[(0, 0), (50, 20), (0, 0)]]
        with pytest.raises(HostRoute):
            nj.print_scaffolds(paths, cuts, n=1, agp=True)
        monkeypatch.setattr(nj, "_write_path_host", host)
        files = nj.print_scaffolds(paths, cuts, n=1, agp=True)
        assert read(files["path"]).decode("ascii").splitlines()[1] == "ntJoin0\t1_f+:0-1981 20N 2_f+:50-20 20N 2_f+:100-2329"
    finally:
        nj.close()


# ---- the families of tests/golden/scaffolds/families: the reference's own .path, write_agp and write_agp_unassigned -----------------

assert NAMES == pin.AGP_NAME_IDS
PIN_CASES = pin.all_cases()


@pytest.mark.parametrize("family,name", PIN_CASES, ids=[f"{family}-{name}" for family, name in PIN_CASES])
def test_families_pinned_to_reference(family, name, tmp_path):
    """write_paths with the strips write_scaffolds returned: the reference's .path and AGP bytes over the paths the writer accepts (with
    the unassigned lines where it accepts all), and for every path whose recorded interval is inverted a refusal that names it"""
    entry = pin.load_family(family)[name]
    case, paths = entry["case"], entry["paths"]
    index = {rid: r for r, (rid, _) in enumerate(case["records"])}
    rows, first = cases.rows_of(paths, index)
    refused = pin.refused_nodes(entry)
    keep = [q for q in range(len(paths)) if q not in refused]
    with MxEngine(k=15, w=10) as e:
        a = e.add_records("t", 1.0, case["records"])
        res = e.write_scaffolds(a, rows, first, overlap_gap=case["overlap_gap"], assigned=str(tmp_path / "s.fa"), unassigned=str(tmp_path / "s.un.fa"),
                                bed=str(tmp_path / "s.bed"))
        leads, tails = res["lead_strip"].tolist(), res["tail_strip"].tolist()
        got = write(e, a, [paths[q] for q in keep], [leads[q] for q in keep], [tails[q] for q in keep], tmp_path / "kept", index)
        assert got == tuple(text.encode("ascii") for text in pin.renumbered(entry, keep))
        if not refused:
            got = write(e, a, paths, leads, tails, tmp_path / "all", index, unassigned=True)
            assert got == (entry["path"].encode("ascii"), (entry["agp"] + entry["agp_unassigned"]).encode("ascii"))
        for q, i in refused.items():
            sub = [x for x in keep if x < q] + [q]
            with pytest.raises(MxError, match=f"path {len(sub) - 1} node {i}: the adjusted interval is empty or inverted") as ei:
                write(e, a, [paths[x] for x in sub], [leads[x] for x in sub], [tails[x] for x in sub], tmp_path / f"refused{q}", index)
            assert ei.value.code == EINVAL and not os.path.exists(tmp_path / f"refused{q}.path") and not os.path.exists(tmp_path / f"refused{q}.agp")
