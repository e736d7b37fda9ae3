"""CPU tests of the lift of features through a piece table (include/ntjoin_mx.h, row f15): the code of the device route
(ntjoin_amd/csrc/lift.h) run serially on the host by tools/lift_check.cpp, built plainly and with AddressSanitizer +
UndefinedBehaviorSanitizer (the runtime linked into the program; nothing is preloaded), against the restatement of the contract
(tests/_lift_restatement.py) on the hand-made cases, a seeded fuzz of tables -- composed ones among them -- and the refusals of
tests/_lift_cases.py; the restatement itself pinned by cases worked by hand; in every case a part spells in the scaffold what its
stretch of the feature spells in the source; the exported symbols, the layouts the Python side mirrors, and the options of the command
line and of the make front-end."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

from tests import _lift_cases as cases, _lift_restatement as R
from tests.conftest import REPO

CSRC = os.path.join(REPO, "ntjoin_amd", "csrc")


def _sanitizer_flags(cxx, td):
    probe = td / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"]):
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] + static
        exe = td / "probe"
        if subprocess.run([cxx] + flags + [str(probe), "-o", str(exe)], capture_output=True).returncode == 0 and \
                subprocess.run([str(exe)], capture_output=True).returncode == 0:
            return flags
    return None


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    td = tmp_path_factory.mktemp("lift_check_" + request.param)
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    extra = []
    if request.param == "sanitized":
        extra = _sanitizer_flags(cxx, td)
        if extra is None:
            pytest.skip("the host compiler has no AddressSanitizer runtime to link")
    out = td / "lift_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror"] + extra +
                          ["-I", os.path.join(REPO, "include"), "-I", CSRC, os.path.join(REPO, "tools", "lift_check.cpp"), "-o", str(out)])
    return str(out)


def _run_intervals(exe, table, source_length, features, tmp_path, whole_only=False):
    f = tmp_path / "case.txt"
    f.write_text(cases.table_text(table, source_length) + "\n" + " ".join([str(len(features))] + [" ".join(map(str, x)) for x in features]) + "\n")
    return subprocess.run([exe, "intervals", str(f)] + (["whole"] if whole_only else []), capture_output=True, text=True, timeout=120)


def _parse(stdout):
    statuses, part_first, parts = [], [0], []
    for line in stdout.splitlines():
        v = [int(x) for x in line.split()]
        assert len(v) == 2 + 5 * v[1]
        statuses.append(v[0])
        parts.extend(tuple(v[2 + 5 * j:7 + 5 * j]) for j in range(v[1]))
        part_first.append(len(parts))
    return statuses, part_first, parts


def _run_bed(exe, table, source_length, source_names, scaffold_names, data, tmp_path, whole_only=False):
    (tmp_path / "table.txt").write_text(cases.table_text(table, source_length) + "\n")
    (tmp_path / "names.txt").write_bytes(b"".join(n + b"\n" for n in list(source_names) + list(scaffold_names)))
    (tmp_path / "in.bed").write_bytes(data)
    r = subprocess.run([exe, "bed"] + [str(tmp_path / n) for n in ("table.txt", "names.txt", "in.bed", "lifted.bed", "unlifted.bed")] +
                       (["whole"] if whole_only else []), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    v = [int(x) for x in r.stdout.split()]
    stats = dict(zip(("lines", "skipped", "features", "whole", "split", "partial", "lost", "invalid", "unknown", "parts", "lifted_bytes",
                      "unlifted_bytes"), v))
    return (tmp_path / "lifted.bed").read_bytes(), (tmp_path / "unlifted.bed").read_bytes(), stats


# ---- the restatement, pinned ---------------------------------------------------------------------------------------------------------
def test_restatement_on_cases_worked_by_hand():
    "a forward piece behind a gap, a reverse piece, a feature across two records of the table: every number from the contract's text"
    F, V, G = R.FWD, R.REV, R.GAP
    table = [[(0, 0, 7, G), (0, 10, 30, F)], [(0, 30, 60, V)]]
    # forward: off = 7, [7 + 12 - 10, 7 + 20 - 10)
    assert R.lift_one(table, [100], (0, 12, 20)) == (R.WHOLE, [(0, 9, 17, 12, 0)])
    # reverse: off = 0, [0 + 60 - 50, 0 + 60 - 35): the feature's last base comes first
    assert R.lift_one(table, [100], (0, 35, 50)) == (R.WHOLE, [(1, 10, 25, 35, 1)])
    # across: [25, 30) of the forward piece, then [30, 40) of the reverse one; nothing is lost: SPLIT
    assert R.lift_one(table, [100], (0, 25, 40)) == (R.SPLIT, [(0, 22, 27, 25, 0), (1, 20, 30, 30, 1)])
    # [5, 10) lies in no piece: PARTIAL; [60, 70) in none at all: LOST; b past the record: INVALID
    assert R.lift_one(table, [100], (0, 5, 12)) == (R.PARTIAL, [(0, 7, 9, 10, 0)])
    assert R.lift_one(table, [100], (0, 60, 70)) == (R.LOST, [])
    assert R.lift_one(table, [100], (0, 60, 101)) == (R.INVALID, [])


@pytest.mark.parametrize("name", sorted(cases.HAND))
def test_restatement_on_the_hand_made_table(name):
    feature, status, parts = cases.HAND[name]
    assert R.lift_one(cases.TABLE, cases.SOURCE_LEN, feature) == (status, parts)


def test_restatement_bed_lines_worked_by_hand():
    table, length, src, dst = [[(0, 10, 30, R.REV)]], [100], [b"c", b"c"], [b"S"]
    bed = b"#x\nc\t12\t20\tg\t0\t+\tmore\r\nc\t12\t20\nc\t5\t12\tp\nq\t1\t2\nc\t1\t12345678901\nc\t12\t20\tg\t0\t-"
    lifted, unlifted, st = R.lift_bed(table, length, src, dst, bed)
    assert lifted == b"S\t10\t18\tg\t0\t-\tmore\nS\t10\t18\nS\t18\t20\tp\nS\t10\t18\tg\t0\t+\n"
    assert unlifted == b"#Partially deleted in new\nc\t5\t12\tp\n#Unknown record\nq\t1\t2\n#Invalid\nc\t1\t12345678901\n"
    assert (st["lines"], st["skipped"], st["features"], st["whole"], st["partial"], st["unknown"], st["invalid"], st["parts"]) == (7, 1, 6, 3, 1, 1, 1, 4)


# ---- lift_check against the restatement -----------------------------------------------------------------------------------------------
def test_hand_made_cases(exe, tmp_path):
    features = [cases.HAND[name][0] for name in sorted(cases.HAND)]
    for whole_only in (False, True):
        want = R.lift(cases.TABLE, cases.SOURCE_LEN, features, whole_only)
        cases.check_spelling(cases.TABLE, cases.SOURCE_LEN, features, *want, whole_only=whole_only)
        r = _run_intervals(exe, cases.TABLE, cases.SOURCE_LEN, features, tmp_path, whole_only)
        assert r.returncode == 0, r.stderr
        assert _parse(r.stdout) == want
    assert want[0] == [cases.HAND[name][1] for name in sorted(cases.HAND)]


def test_seeded_fuzz(exe, tmp_path):
    composed = 0
    for seed in range(210):
        table, source_length, features = cases.fuzz_case(seed)
        composed += seed % 3 != 1
        want = R.lift(table, source_length, features, whole_only=seed % 7 == 0)
        cases.check_spelling(table, source_length, features, *want, seed=seed, whole_only=seed % 7 == 0)
        r = _run_intervals(exe, table, source_length, features, tmp_path, whole_only=seed % 7 == 0)
        assert r.returncode == 0, (seed, r.stderr)
        assert _parse(r.stdout) == want, seed
    assert composed >= 100


@pytest.mark.parametrize("long_at,n_short", cases.CARRY_CASES)
def test_lookups_behind_a_long_piece(exe, tmp_path, long_at, n_short):
    "the tables of tests/test_gpu_lift.py::test_lookups_that_live_on_the_carries: the header's two bisections on the host at these sizes"
    table, source_length, features, statuses = cases.carry_case(long_at, n_short)
    want = cases.carry_expected(long_at, n_short)
    assert want[0] == statuses
    if n_short < 10000:
        cases.check_spelling(table, source_length, features, *want)
    r = _run_intervals(exe, table, source_length, features, tmp_path)
    assert r.returncode == 0, r.stderr
    assert _parse(r.stdout) == want


def test_no_records_no_sequence_pieces_no_features(exe, tmp_path):
    for table, features in (([], [(0, 0, 5)]), ([[(0, 0, 5, R.GAP)]], [(0, 0, 5), (1, 0, 1)]), (cases.TABLE, [])):
        want = R.lift(table, cases.SOURCE_LEN, features)
        r = _run_intervals(exe, table, cases.SOURCE_LEN, features, tmp_path)
        assert r.returncode == 0 and _parse(r.stdout) == want
        assert set(want[0]) <= {R.LOST}


@pytest.mark.parametrize("name", sorted(cases.REFUSED))
def test_refusals(exe, name, tmp_path):
    table, source_length, code = cases.REFUSED[name]
    with pytest.raises(R.Refused) as ei:
        R.lift(table, source_length, [(0, 0, 1)])
    assert ei.value.code == code
    r = _run_intervals(exe, table, source_length, [(0, 0, 1)], tmp_path)
    assert r.returncode == {R.EINVAL: 3, R.ELIMIT: 4}[code] and r.stderr.strip() and not r.stdout
    if code == R.EINVAL:
        assert re.search(r"table record \d+", r.stderr)


@pytest.mark.parametrize("whole_only", [False, True])
def test_bed_file(exe, tmp_path, whole_only):
    want = R.lift_bed(cases.TABLE, cases.SOURCE_LEN, cases.SOURCE_NAMES, cases.SCAFFOLD_NAMES, cases.BED, whole_only)
    got = _run_bed(exe, cases.TABLE, cases.SOURCE_LEN, cases.SOURCE_NAMES, cases.SCAFFOLD_NAMES, cases.BED, tmp_path, whole_only)
    assert got == want
    st = want[2]
    assert st["skipped"] == 6 and all(st[k] > 0 for k in ("whole", "split", "partial", "lost", "invalid", "unknown"))
    if not whole_only:
        assert b"ntJoin0\t670\t770\tgeneB\t0\t-\n" in want[0] and b"ntJoin0\t670\t770\tgeneC\t0\t.\n" in want[0]
        assert b"ntJoin0\t350\t400\tsplit\t0\t+\nntJoin1\t0\t100\tsplit\t0\t+\n" in want[0]
        assert b"ntJoin0\t670\t770\tgeneD\t960\t-\t120\t180\t0,0,255\t2\t10,20\t0,80\n" in want[0]
        assert b"ntJoin0\t10\t50\t\n" in want[0] and want[0].endswith(b"ntJoin1\t605\t905\tlast\t0\t+\n")
        assert b"#Split in new\nctg0\t350\t500\tsplit\t0\t+\n" in want[1]


def test_bed_fuzz(exe, tmp_path):
    rng = cases.random.Random(99)
    for seed in range(0, 60, 2):
        table, source_length, features = cases.fuzz_case(seed, n_features=25)
        src = [b"s%d" % (r % 4 if seed % 4 == 0 else r) for r in range(len(source_length))]   # (duplicate names now and then)
        dst = [b"ntJoin%d" % r for r in range(len(table))]
        lines = []
        for r, a, b in features:
            name = src[r] if r < len(src) else b"nowhere"
            tail = rng.choice((b"", b"\tx", b"\tx\t0\t+", b"\tx\t0\t-", b"\tx\t0\t.\t1\t2", b"\t\t\t+\t"))
            lines.append(name + b"\t%d\t%d" % (a, b) + tail + rng.choice((b"\n", b"\n", b"\r\n")))
            if rng.random() < 0.1:
                lines.append(rng.choice((b"\n", b"#c\n", b"track\n", b"x\t1\n", b"x\ty\tz\n")))
        data = b"".join(lines)
        if seed % 3 == 0:
            data = data.rstrip(b"\r\n")
        assert _run_bed(exe, table, source_length, src, dst, data, tmp_path) == R.lift_bed(table, source_length, src, dst, data), seed


# ---- the library's surface ----------------------------------------------------------------------------------------------------------------
def test_symbols_constants_and_layouts():
    import numpy as np
    from ntjoin_amd import capi
    from ntjoin_amd.engine import MxEngine
    for name in ("mxg_lift_prepare", "mxg_lift_intervals", "mxg_lift_bed"):
        assert name in capi.SYMBOLS
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in ("mxg_lift_prepare", "mxg_lift_intervals", "mxg_lift_bed"):
        assert getattr(lib, name)
    header = open(os.path.join(REPO, "include", "ntjoin_mx.h"), encoding="utf-8").read()
    for name, value in (("WHOLE", R.WHOLE), ("SPLIT", R.SPLIT), ("PARTIAL", R.PARTIAL), ("LOST", R.LOST), ("INVALID", R.INVALID), ("UNKNOWN", R.UNKNOWN)):
        assert f"#define MXG_LIFT_{name} {value}u" in header and getattr(capi, "LIFT_" + name) == value
    assert "#define MXG_LIFT_WHOLE_ONLY 0x1u" in header and capi.LIFT_WHOLE_ONLY == 1
    # the layouts: the header's fields in order, 8 bytes each (api.cpp asserts the sizes)
    view = re.search(r"typedef struct mxg_lift_view \{(.*?)\} mxg_lift_view;", header, re.S).group(1)
    names = re.findall(r"\*?(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", view))
    assert names == [f[0] for f in capi.LiftView._fields_] and ctypes.sizeof(capi.LiftView) == 72
    stats = re.search(r"typedef struct mxg_lift_stats \{(.*?)\} mxg_lift_stats;", header, re.S).group(1)
    assert re.findall(r"(\w+)(?:\[6\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", stats)) == ["lines", "skipped", "features", "status", "parts", "lifted_bytes", "unlifted_bytes"]
    assert ctypes.sizeof(capi.LiftStats) == 96 and capi.LIFT_STATS_FIELDS[3:9] == ("whole", "split", "partial", "lost", "invalid", "unknown")
    assert MxEngine.LIFT_PART.names == ("s_record", "s_start", "s_end", "src_start", "reverse")
    assert np.dtype(MxEngine.LIFT_PART).itemsize == 17
    for method in ("lift_prepare", "lift_intervals", "lift_bed"):
        assert callable(getattr(MxEngine, method))


# ---- command line and make front-end -----------------------------------------------------------------------------------------------------
def test_command_line_takes_the_lift_options():
    from ntjoin_amd import run
    tail = ["-s", "tgt.fa.k32.w100.tsv", "-r", "2", "-p", "pre", "-k", "32", "ref.fa.k32.w100.tsv"]
    args = run.parse_arguments(["--lift", "a.bed", "dir/b.genes.bed", "--lift_whole_only"] + tail)
    assert args.lift == ["a.bed", "dir/b.genes.bed"] and args.lift_whole_only is True and args.FILES == ["ref.fa.k32.w100.tsv"]
    args = run.parse_arguments(tail + ["--lift", "a.bed"])
    assert args.lift == ["a.bed"] and args.lift_whole_only is False
    args = run.parse_arguments(tail)
    assert args.lift == [] and args.lift_whole_only is False
    from ntjoin_amd.ntjoin import Ntjoin, lift_outputs
    assert lift_outputs("pre", "dir/b.genes.bed") == ("pre.b.genes.lifted.bed", "pre.b.genes.unlifted.bed")
    assert lift_outputs("out/pre", "a.txt") == ("out/pre.a.txt.lifted.bed", "out/pre.a.txt.unlifted.bed")
    for method in ("lift_prepare", "lift_bed", "lift_beds"):
        assert callable(getattr(Ntjoin, method))
    r = subprocess.run([sys.executable, "-m", "ntjoin_amd.assemble", "--help"], capture_output=True, text=True, cwd=REPO)
    assert r.returncode == 0 and "--lift" in r.stdout and "--lift_whole_only" in r.stdout


def test_make_front_end_forwards_the_lift_options():
    def dry(*words):
        res = subprocess.run(["make", "-n", "-f", os.path.join(REPO, "ntJoin-mx"), "scaffold", "target=t.fa", "references=r.fa", "reference_weights=2",
                              "k=32", "w=100", *words], capture_output=True, text=True, check=True, timeout=60)
        return " ".join(res.stdout.replace("\\\n", " ").split())
    plain = dry()
    assert "--lift" not in plain and dry("lift=", "lift_whole_only=False") == plain
    # the list of files ends at the next option, in front of the positional sketches
    assert "python3 -m ntjoin_amd.assemble --lift a.bed b.bed --lift_whole_only -p " in dry("lift=a.bed b.bed", "lift_whole_only=True")
    one = dry("lift=genes.bed")
    assert "python3 -m ntjoin_amd.assemble --lift genes.bed -p " in one and "--lift_whole_only" not in one
    assert "--lift a.bed -p " in dry("lift=a.bed", "rounds_w=50") and '--rounds_w "50"' in dry("lift=a.bed", "rounds_w=50")
