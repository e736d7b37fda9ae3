"""CPU tests of the synteny blocks (include/ntjoin_mx.h, row f12): the restatement of the contract (tests/_synteny_restatement.py)
pinned by blocks derived by hand; the code of the device route (ntjoin_amd/csrc/synteny.h) run serially on the host by
tools/synteny_check.cpp, built plainly and with AddressSanitizer + UndefinedBehaviorSanitizer (the runtime linked into the program;
nothing is preloaded), against the restatement on the hand-made cases, the shapes by size and the seeded fuzz of
tests/_synteny_cases.py; the PAF line of a block; the exported symbols, the layouts the Python side mirrors and the command line."""
import os
import random
import re
import shutil
import subprocess

import pytest

from tests import _synteny_cases as cases, _synteny_restatement as R
from tests.conftest import REPO

CSRC = os.path.join(REPO, "ntjoin_amd", "csrc")
HAND = cases.hand_cases()


def restated(case):
    vpos, vrec = cases.graph_arrays(case)
    return R.synteny(vpos, vrec, case["q"], case["s"], case["k"], case["max_gap"], case["min_anchors"], case["min_span"], case["pieces"],
                     case["first"])


# ---- the restatement against blocks derived by hand --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND))
def test_restatement_gives_the_blocks_derived_by_hand(name):
    case = HAND[name]
    got = restated(case)
    assert got["blocks"] == case["expect"]
    assert (got["n_anchors_total"], got["n_links"]) == (case["n_anchors_total"], case["n_links"])


def test_hand_cases_cover_what_the_contract_names():
    "a turning point in two blocks, max_gap and one more, a REV piece, both piece borders, an anchor in two pieces and one in none"
    turn = HAND["turning_point"]["expect"]
    assert turn[0][3] - 32 == turn[1][2] == 300 and turn[0][7] == 0 and turn[1][7] == 1
    assert HAND["max_gap_border"]["max_gap"] == 1000 and len(HAND["max_gap_border"]["expect"]) == 2
    assert HAND["rev_piece"]["pieces"][0][3] == R.REV and HAND["rev_piece"]["expect"][0][7] == 1
    borders = HAND["piece_borders"]
    assert [(p[1], p[2]) for p in borders["pieces"]] == [(100, 232), (101, 332), (100, 231)]   # a == qpos, qpos + k == b; a == qpos + 1; b - 1
    assert borders["n_anchors_total"] == 5   # 4 vertices: two appear twice, one vanishes, one lies in one piece


def test_anchor_list_of_a_table_record_by_record():
    case = HAND["gap_and_offsets"]
    vpos, vrec = cases.graph_arrays(case)
    assert R.anchor_list(vpos, vrec, 1, 0, 32, case["pieces"], case["first"]) == [(0, 0, 0, 1000), (0, 100, 0, 2000), (0, 210, 0, 3000)]
    assert R.query_lengths(case["lengths"][1], case["pieces"], case["first"]) == [132 + 10 + 150]
    case = HAND["piece_borders"]
    vpos, vrec = cases.graph_arrays(case)
    assert R.anchor_list(vpos, vrec, 1, 0, 32, case["pieces"], case["first"]) == \
        [(0, 0, 0, 1000), (0, 100, 0, 2000), (1, 99, 0, 2000), (1, 199, 0, 3000), (2, 0, 0, 1000)]


def test_paf_line_of_a_block():
    "12 columns and the cm tag; matches = min(n k, spans), blocklen = max(spans)"
    assert R.paf_line((3, 0, 100, 332, 0, 1000, 3032, 0), "ntJoin0", 5000, "chr1", 90000, 32) == \
        "ntJoin0\t5000\t100\t332\t+\tchr1\t90000\t1000\t3032\t96\t2032\t255\tcm:i:3\n"
    assert R.paf_line((2, 1, 99, 131, 4, 20, 52, 1), "c:0-9", 200, "t", 60, 32) == "c:0-9\t200\t99\t131\t-\tt\t60\t20\t52\t32\t32\t255\tcm:i:2\n"
    case = HAND["record_borders"]
    text = R.paf(case["expect"], ["q0", "q1"], [100, 200], ["s0", "s1"], [300, 700], 32)
    assert text.splitlines()[1] == "q0\t100\t30\t72\t+\ts1\t700\t300\t432\t42\t132\t255\tcm:i:2"
    assert text.count("\n") == 4


# ---- tools/synteny_check: the device route's code on the host ------------------------------------------------------------------------
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
    td = tmp_path_factory.mktemp("synteny_check_" + request.param)
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    extra = []
    if request.param == "sanitized":
        extra = _sanitizer_flags(cxx, td)
        if extra is None:
            pytest.skip("the host compiler has no AddressSanitizer runtime to link")
    out = td / "synteny_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror"] + extra +
                          ["-I", os.path.join(REPO, "include"), "-I", CSRC, os.path.join(REPO, "tools", "synteny_check.cpp"), "-o", str(out)])
    return str(out)


def _input_text(case):
    vpos, vrec = cases.graph_arrays(case)
    q, s = case["q"], case["s"]
    anchors = [(vrec[q][v], vpos[q][v], vrec[s][v], vpos[s][v]) for v in range(len(vpos[q]))]
    random.Random(5).shuffle(anchors)   # (the program sorts, as the sketch is sorted)
    words = [case["k"], case["max_gap"], case["min_anchors"], case["min_span"], len(case["lengths"][q])] + list(case["lengths"][q])
    words += [len(anchors)] + [x for a in anchors for x in a]
    if case["pieces"] is None:
        words.append(0)
    else:
        first = case["first"]
        words += [1, len(first) - 1]
        for r in range(len(first) - 1):
            rows = case["pieces"][first[r]:first[r + 1]]
            words += [len(rows)] + [x for row in rows for x in row]
    return " ".join(str(int(w)) for w in words) + "\n"


def _run(exe, case, tmp_path):
    f = tmp_path / "case.txt"
    f.write_text(_input_text(case))
    return subprocess.run([exe, str(f)], capture_output=True, text=True, timeout=120)


def _check(exe, case, tmp_path):
    want = restated(case)
    res = _run(exe, case, tmp_path)
    assert res.returncode == 0, res.stderr
    lines = [[int(x) for x in line.split()] for line in res.stdout.splitlines()]
    assert lines[0] == [want["n_anchors_total"], want["n_links"]]
    assert [tuple(v[:8]) for v in lines[1:]] == want["blocks"]
    k = case["k"]
    for v in lines[1:]:
        assert v[8] == min(v[0] * k, v[3] - v[2], v[6] - v[5]) and v[9] == max(v[3] - v[2], v[6] - v[5])


@pytest.mark.parametrize("name", sorted(HAND))
def test_check_program_on_the_hand_cases(exe, name, tmp_path):
    _check(exe, HAND[name], tmp_path)


def test_check_program_on_shapes(exe, tmp_path):
    for case in (cases.line_case(2), cases.line_case(257), cases.line_case(257, reverse=True), cases.zigzag_case(65), cases.nolink_case(64),
                 cases.from_anchors([]), cases.from_anchors([(0, 5, 0, 5)]), cases.mixed_case(1025, seed=3, max_gap=1000, min_anchors=3)):
        _check(exe, case, tmp_path)
    rng = random.Random(11)
    case = cases.mixed_case(3000, seed=4)
    case["pieces"], case["first"] = cases.pieces_of(case, rng, many=1000)
    assert case["first"][1] - case["first"][0] >= 1000
    _check(exe, case, tmp_path)


def test_check_program_on_the_fuzz(exe, tmp_path):
    seen_blocks = seen_tables = seen_reverse = 0
    for i in range(cases.FUZZ_CASES):
        case = cases.fuzz_case(i)
        _check(exe, case, tmp_path)
        want = restated(case)
        seen_blocks += len(want["blocks"])
        seen_reverse += sum(b[7] for b in want["blocks"])
        seen_tables += case["pieces"] is not None
    assert seen_blocks > 200 and seen_reverse > 20 and seen_tables == cases.FUZZ_CASES // 2


def test_check_program_refuses_what_the_contract_refuses(exe, tmp_path):
    base = HAND["rev_piece"]
    for pieces, first, status, word in (([(0, 50, 5000, R.REV)], [0, 1], 3, "not inside"), ([(0, 60, 60, R.FWD)], [0, 1], 3, "empty or inverted"),
                                        ([(7, 0, 10, R.FWD)], [0, 1], 3, "does not exist"), ([(0, 0, 10, 3)], [0, 1], 3, "unknown kind"),
                                        ([(0, 0, 10, R.FWD)], [0, 1, 1], 3, "no pieces"),
                                        ([(0, 0, 2 ** 32 - 1, R.GAP), (0, 0, 1, R.GAP)], [0, 2], 4, "longer than 2^32 - 1")):
        res = _run(exe, dict(base, pieces=pieces, first=first), tmp_path)
        assert res.returncode == status and word in res.stderr, (pieces, res.returncode, res.stderr)
    res = _run(exe, dict(base, pieces=None, first=None, min_anchors=1), tmp_path)
    assert res.returncode == 3 and "at least two" in res.stderr


# ---- the surface ----------------------------------------------------------------------------------------------------------------------
def test_symbols_and_layouts():
    import ctypes as C

    from ntjoin_amd import capi
    header = open(os.path.join(REPO, "include", "ntjoin_mx.h"), encoding="utf-8").read()
    for name in ("mxg_synteny_blocks", "mxg_write_synteny_paf"):
        assert name in capi.SYMBOLS and re.search(r"\bint " + name + r"\(", header)
    assert C.sizeof(capi.SyntenyParams) == 16 and C.sizeof(capi.SyntenyView) == 88
    api = open(os.path.join(CSRC, "api.cpp"), encoding="utf-8").read()
    assert "sizeof(mxg_synteny_params) == 16" in api and "sizeof(mxg_synteny_view) == 88" in api


def test_command_line_flags():
    from ntjoin_amd.run import parse_arguments
    argv = ["-s", "t.fa.k32.w100.tsv", "-r", "1", "-k", "32", "r.fa.k32.w100.tsv"]
    off = parse_arguments(argv)
    assert off.synteny is False and off.synteny_max_gap == 100000 and off.synteny_min_anchors == 3 and off.synteny_min_span == 0
    on = parse_arguments(argv + ["--synteny", "--synteny_max_gap", "0", "--synteny_min_anchors", "2", "--synteny_min_span", "500"])
    assert on.synteny is True and (on.synteny_max_gap, on.synteny_min_anchors, on.synteny_min_span) == (0, 2, 500)


def test_make_front_end_hands_the_flags_on():
    def dry(*extra):
        res = subprocess.run([os.path.join(REPO, "ntJoin-mx"), "-n", "scaffold", "target=t.fa", "references=r.fa", "reference_weights=2"] + list(extra),
                             capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        return res.stdout
    plain, on = dry(), dry("synteny=True")
    assert "--synteny" not in plain
    assert " --synteny --synteny_max_gap 100000 --synteny_min_anchors 3" in on
    assert on.replace(" --synteny --synteny_max_gap 100000 --synteny_min_anchors 3", "") == plain
    assert " --synteny --synteny_max_gap 0 --synteny_min_anchors 2" in dry("synteny=True", "synteny_max_gap=0", "synteny_min_anchors=2")
