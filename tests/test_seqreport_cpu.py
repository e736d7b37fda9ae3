"""CPU tests of the assembly report: the code of the device route (ntjoin_amd/csrc/seqstat.h) run on the host by
tools/seqstat_check.cpp -- serially, cut into pieces with the states composed, and with the compositions regrouped -- built with
AddressSanitizer + UndefinedBehaviorSanitizer (the runtime linked into the program; nothing is preloaded) against the restatement
(tests/_seqreport_restatement.py); the contiguity block against a brute-force version; --report on the command line and in
`ntJoin-mx scaffold`; the exported symbols.  The same program over the scaffold files of the window route's shapes
(tests/_seqreport_cases.py window_shapes)."""
import os
import shutil
import subprocess

import pytest

from ntjoin_amd import capi
from ntjoin_amd.run import parse_arguments
from tests import _seqreport_cases as cases, _seqreport_restatement as R
from tests.conftest import GOLDEN, REPO

CSRC = os.path.join(REPO, "ntjoin_amd", "csrc")
PARAMS = [(mg, ml) for mg in (1, 2, 10) for ml in (0, 500)]


def _sanitizer_flags(cxx, td):
    probe = td / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] + static
        exe = td / "probe"
        if subprocess.run([cxx] + flags + [str(probe), "-o", str(exe)], capture_output=True).returncode == 0 and \
                subprocess.run([str(exe)], capture_output=True).returncode == 0:
            return flags
    return []  # (a compiler without the runtime: the program is checked without it)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    td = tmp_path_factory.mktemp("seqstat_check")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    out = td / "seqstat_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror"] + _sanitizer_flags(cxx, td) +
                          ["-I", CSRC, os.path.join(REPO, "tools", "seqstat_check.cpp"), "-o", str(out)])
    return str(out)


def _parse(stdout):
    got = {}
    for line in stdout.decode().splitlines():
        key, *words = line.split()
        got[key] = [int(w) for w in words]
    return got


def _check(exe, text, tmp_path, seed):
    fa = tmp_path / "x.fa"
    fa.write_bytes(text)
    cuts = "every" if len(text) <= 700 else f"rand:{seed}:48"
    for mg, ml in PARAMS:
        r = subprocess.run([exe, str(fa), str(mg), str(ml), cuts], capture_output=True, timeout=120)
        assert r.returncode == 0, (mg, ml, r.stdout[-300:], r.stderr[-2000:])  # (1: the three walks disagree)
        got, want = _parse(r.stdout), R.report(text, mg, ml)
        assert got["records"] == [want["n_records"]] and got["bases"] == [want["bases"]]
        assert got["counts"] == [want[k] for k in ("a", "c", "g", "t", "n", "other", "lower")]
        assert got["gaps"] == want["gap_len"] and got["contigs"] == want["contig_len"]
        assert got["scaffold"] == [want["scaffold"][k] for k in R.BLOCK]
        assert got["contig"] == [want["contig"][k] for k in R.BLOCK]


@pytest.mark.parametrize("name", sorted(os.listdir(os.path.join(GOLDEN, "fasta"))))
def test_host_program_on_the_goldens(exe, tmp_path, name):
    with open(os.path.join(GOLDEN, "fasta", name), "rb") as fh:
        _check(exe, fh.read(), tmp_path, 7)


SHAPES = cases.shapes()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_host_program_equals_restatement_on_shapes(exe, tmp_path, name):
    _check(exe, SHAPES[name], tmp_path, 11)


WINDOW_SHAPES = cases.window_shapes()


@pytest.mark.parametrize("name", sorted(WINDOW_SHAPES))
def test_host_program_equals_restatement_on_the_window_shapes(exe, tmp_path, name):
    """the scaffold files the restatement expects of the window route's shapes (tests/test_gpu_report_windows.py), through the lane
    code on the host: the report's restatement and seqstat.h agree on exactly these texts before the GPU is asked"""
    for fold in (False, True) if name in cases.FOLD_TOO else (False,):
        assigned, unassigned = cases.window_texts(WINDOW_SHAPES[name], fold)
        assert assigned.startswith(b">ntJoin0\n")
        for seed, text in enumerate((assigned, unassigned, assigned + unassigned), 13):
            _check(exe, text, tmp_path, seed)
    if name.startswith("empty_files"):
        want = R.report(unassigned)
        assert unassigned == b"" and want["gap_len"] == want["contig_len"] == [] and want["scaffold"] == dict.fromkeys(R.BLOCK, 0)
        assert not any(want[k] for k in ("n_records", "bases", "a", "c", "g", "t", "n", "other", "lower", "n_gaps", "gap_bases", "max_gap"))


def test_host_program_on_a_tile_of_line_ends(exe, tmp_path):
    text = cases.line_end_tile()
    _check(exe, text, tmp_path, 17)
    assert R.report(text)["gap_len"] == [25]


def test_cuts_at_every_offset_of_a_small_file(exe, tmp_path):
    "every byte a piece of its own: runs, borders, line ends and headers all fall on cuts"
    text = b">a\nNNNNNACGTNNNNNNNNNNNNAC\nGTNN\r\nNNNNNNNNnnACGT\n>b desc\n>c\nNNNNNNNNNNNN\n>d\nACNNNNNNNNNGT\nA\n>e\nnnnnnnnnnnT"
    assert len(text) <= 700
    _check(exe, text, tmp_path, 1)
    want = R.report(text)
    assert want["gap_len"] == [10, 12, 12, 12] and want["contig_len"] == [1, 4, 4, 9, 14]


def _brute(lengths, min_len):
    "Nx by expanding every length into its bases: the length that holds base ceil(x sum / 100) of the descending order"
    sel = sorted((x for x in lengths if x >= min_len), reverse=True)
    block = dict.fromkeys(R.BLOCK, 0)
    block["n"] = len(lengths)
    if sel:
        total = sum(sel)
        block.update(n_min=len(sel), sum=total, min=min(sel), max=max(sel))
        for x in (50, 75, 90):
            need = -(-x * total // 100)
            acc = 0
            for j, length in enumerate(sel, 1):
                acc += length
                if acc >= need:
                    block[f"n{x}"], block[f"l{x}"] = length, j
                    break
    return block


@pytest.mark.parametrize("lengths,min_len", [
    ([2, 2, 2, 2], 0),                     # a tie at the N50 border: exactly half after two
    ([5, 5, 5, 5, 4, 4, 4, 4, 4], 0),      # ties around N75 and N90
    ([10, 9, 1], 0), ([10, 9, 1], 9), ([3, 1, 1, 1], 0),
    ([700], 500), ([700], 0),              # one length
    ([], 0), ([], 500),                    # no length
    ([499, 1, 20], 500),                   # all below min_len
    ([2 ** 33, 2 ** 33 + 7, 2 ** 32, 5], 500), ([2 ** 40 + 1] * 9 + [2 ** 36], 0),  # sums above 2^32
    ([(7 * i * i + 3) % 1000 for i in range(300)], 100),
])
def test_contiguity_block_against_brute_force(exe, lengths, min_len):
    r = subprocess.run([exe, "--contig", str(min_len)] + [str(x) for x in lengths], capture_output=True, timeout=60)
    assert r.returncode == 0, r.stderr
    want = _brute(lengths, min_len)
    assert _parse(r.stdout)["block"] == [want[k] for k in R.BLOCK]
    assert R.contiguity(lengths, min_len) == want


# ---- surfaces
ARGV = ["-s", "t.fa.k32.w100.tsv", "-r", "2", "-k", "32", "r.fa.k32.w100.tsv"]


def test_parser_accepts_the_three_flags():
    off = parse_arguments(ARGV)
    assert off.report is False and off.report_min_gap == 10 and off.report_min_len == 500
    on = parse_arguments(ARGV + ["--report", "--report_min_gap", "1", "--report_min_len", "0", "--gz", "--fai"])
    assert on.report is True and on.report_min_gap == 1 and on.report_min_len == 0


def dry(*words):
    return subprocess.run(["make", "-n", "-f", os.path.join(REPO, "ntJoin-mx"), "scaffold", "target=t.fa", "references=r.fa", "reference_weights=2",
                           "k=32", "w=100", *words], capture_output=True, text=True, check=True, timeout=60).stdout


def test_make_variable_hands_the_flags_on():
    plain, on = dry(), dry("report=True")
    assert dry("report=False") == plain and "--report" not in plain
    assert " --report --report_min_gap 10 --report_min_len 500" in on
    assert on.replace(" --report --report_min_gap 10 --report_min_len 500", "") == plain
    assert " --report --report_min_gap 3 --report_min_len 0" in dry("report=True", "report_min_gap=3", "report_min_len=0")


def test_symbols_flag_and_struct_are_bound():
    for name in ("mxg_set_report_params", "mxg_assembly_report", "mxg_scaffold_report"):
        assert name in capi.SYMBOLS
    assert capi.SCAF_REPORT == 0x8 and (capi.REPORT_ASSIGNED, capi.REPORT_UNASSIGNED, capi.REPORT_ALL) == (0, 1, 2)
    import ctypes
    assert ctypes.sizeof(capi.SeqReport) == 312 and ctypes.sizeof(capi.Contiguity) == 88
    header = open(os.path.join(REPO, "include", "ntjoin_mx.h"), encoding="utf-8").read()
    assert "#define MXG_SCAF_REPORT 0x8u" in header
