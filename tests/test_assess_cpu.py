"""CPU tests of the assessment (include/ntjoin_mx.h, row f13): the restatement of the contract (tests/_assess_restatement.py) pinned
by chains, breakpoints and sums derived by hand (tests/_assess_cases.py); the code of the device route (ntjoin_amd/csrc/assess.h) run
serially on the host by tools/assess_check.cpp, built plainly and with AddressSanitizer + UndefinedBehaviorSanitizer (the runtime
linked into the program; nothing is preloaded), against the restatement on those cases and on 100 seeded ones; the TSV and BED
formatters against literals; the exported symbol, the layouts the Python side mirrors and the command line."""
import os
import re
import shutil
import subprocess

import pytest

from tests import _assess_cases as AC, _assess_restatement as A, _synteny_cases as cases, _synteny_restatement as R
from tests.conftest import REPO

CSRC = os.path.join(REPO, "ntjoin_amd", "csrc")
BLOCK = AC.block_cases()
ANCHOR = AC.anchor_cases()


def restated(case):
    return A.assess(case["blocks"], case["k"], case["q_len"], case["s_len"], pieces=case["pieces"], first=case["first"], **case["params"])


# ---- the restatement against results derived by hand --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BLOCK))
def test_restatement_gives_what_was_derived_by_hand(name):
    case, expect = BLOCK[name]
    got = restated(case)
    assert AC.matches(got, expect), {key: got[key] for key in expect}
    assert got["n_blocks"] == len(case["blocks"]) and sum(got["breakpoints"].values()) == got["n_breakpoints"] == len(got["bps"]["chain"])
    assert sum(got["chains"]["n_blocks"]) == len(case["blocks"]) and sum(got["chains"]["n_anchors"]) == sum(b[0] for b in case["blocks"])


def test_hand_cases_cover_what_the_contract_names():
    names = set(BLOCK)
    assert {"stray_split", "gq_least", "gq_below", "gs_least", "gs_below", "merge_gap_q", "merge_gap_q_over", "merge_gap_s", "merge_gap_s_over",
            "max_indel", "max_indel_over", "join_indel", "one_piece", "turning_anchor", "translocation", "relocation_order", "record_border",
            "union", "nx", "nx_d_zero", "zero_blocks"} <= names
    turn = restated(BLOCK["turning_anchor"][0])["bps"]
    assert turn["q_lo"][0] > turn["q_hi"][0]
    nx = BLOCK["nx"][0]
    assert 100 * 282 == 50 * sum(nx["q_len"])   # the 50 % mark is met exactly


@pytest.mark.parametrize("name", sorted(ANCHOR))
def test_anchor_cases_spell_the_blocks_they_promise(name):
    "what tests/test_gpu_assess.py feeds the device: the blocks and the expected figures, through both restatements"
    case, expect = ANCHOR[name]
    vpos, vrec = cases.graph_arrays(case)
    syn = R.synteny(vpos, vrec, case["q"], case["s"], case["k"], case["max_gap"], case["min_anchors"], case["min_span"], case["pieces"], case["first"])
    assert len(syn["blocks"]) == case["n_specs"]
    got = A.assess(syn["blocks"], case["k"], R.query_lengths(case["lengths"][case["q"]], case["pieces"], case["first"]), case["lengths"][case["s"]],
                   pieces=case["pieces"], first=case["first"], **case["assess"])
    assert AC.matches(got, expect), {key: got[key] for key in expect}


def test_anchor_cases_hold_the_gaps_of_exactly_one_minus_k():
    "the three boundary cases give the device two blocks whose gap is 1 - k: on the query, on the subject forward, and reverse"
    for name, gap in (("gq_least", lambda a, b: b[2] - a[3]), ("gs_least", lambda a, b: b[5] - a[6]), ("gs_least_reverse", lambda a, b: a[5] - b[6])):
        case, _ = ANCHOR[name]
        vpos, vrec = cases.graph_arrays(case)
        a, b = R.synteny(vpos, vrec, 1, 0, case["k"], case["max_gap"], case["min_anchors"], case["min_span"])["blocks"]
        assert gap(a, b) == 1 - case["k"] and a[7] == b[7] == (name == "gs_least_reverse"), (name, a, b)
        assert case["assess"] == dict(merge_gap=0, max_indel=0)   # (so that only the `>= 1 - k` tests decide)


def test_piece_of_counts_gap_pieces():
    pieces, first = [(0, 0, 200, 0), (0, 0, 50, 2), (0, 200, 950, 0), (1, 0, 10, 1)], [0, 3, 4]
    assert [A.piece_of(pieces, first, 0, x) for x in (0, 199, 200, 249, 250, 999)] == [0, 0, 1, 1, 2, 2]
    assert A.piece_of(pieces, first, 1, 9) == 0 and A.piece_of(None, None, 5, 123) == 0


# ---- tools/assess_check: the device route's code on the host --------------------------------------------------------------------------
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
    td = tmp_path_factory.mktemp("assess_check_" + request.param)
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    extra = []
    if request.param == "sanitized":
        extra = _sanitizer_flags(cxx, td)
        if extra is None:
            pytest.skip("the host compiler has no AddressSanitizer runtime to link")
    out = td / "assess_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror"] + extra +
                          ["-I", os.path.join(REPO, "include"), "-I", CSRC, os.path.join(REPO, "tools", "assess_check.cpp"), "-o", str(out)])
    return str(out)


def _input_text(case):
    p = dict(A.DEFAULTS, **case["params"])
    words = [case["k"], p["merge_gap"], p["max_indel"], p["join_indel"], len(case["q_len"])] + list(case["q_len"])
    words += [len(case["s_len"])] + list(case["s_len"]) + [len(case["blocks"])] + [x for b in case["blocks"] for x in b]
    if case["pieces"] is None:
        words.append(0)
    else:
        first = case["first"]
        words += [1, len(first) - 1]
        for r in range(len(first) - 1):
            rows = case["pieces"][first[r]:first[r + 1]]
            words += [len(rows)] + [row[2] - row[1] for row in rows]
    return " ".join(str(int(w)) for w in words) + "\n"


def _check(exe, case, tmp_path):
    want = restated(case)
    f = tmp_path / "case.txt"
    f.write_text(_input_text(case))
    res = subprocess.run([exe, str(f)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    head = [int(x) for x in lines[0].split()]
    assert head == [want["n_blocks"], want["n_chains"], want["n_breakpoints"]] + [want["breakpoints"][(kind, j)] for kind in range(3) for j in range(2)] + \
        [want[key] for key in ("query_bases", "subject_bases", "aligned_query", "chained_subject", "covered_subject")]
    assert lines[1].startswith("X ")
    assert [int(x) for x in lines[1].split()[1:]] == [want[b][f"{c}{x}"] for b in ("na", "nga", "ng") for x in (50, 75, 90) for c in "nl"]
    chains = [[int(x) for x in line.split()[1:]] for line in lines[2:] if line.startswith("C ")]
    bps = [[int(x) for x in line.split()[1:]] for line in lines[2:] if line.startswith("B ")]
    assert chains == [list(row) for row in zip(*[want["chains"][name] for name in A.CHAIN_FIELDS])]
    assert bps == [list(row) for row in zip(*[want["bps"][name] for name in A.BP_FIELDS])]
    return want


@pytest.mark.parametrize("name", sorted(BLOCK))
def test_check_program_on_the_hand_cases(exe, name, tmp_path):
    _check(exe, BLOCK[name][0], tmp_path)


def test_check_program_on_the_fuzz(exe, tmp_path):
    chains = bps = joins = tables = 0
    kinds = set()
    for i in range(AC.FUZZ_CASES):
        case = AC.fuzz_block_case(i)
        want = _check(exe, case, tmp_path)
        chains += want["n_chains"]
        bps += want["n_breakpoints"]
        joins += sum(want["breakpoints"][(kind, 1)] for kind in range(3))
        kinds |= {kind for (kind, _j), n in want["breakpoints"].items() if n}
        tables += case["pieces"] is not None
    assert chains > 500 and bps > 300 and joins > 20 and kinds == {0, 1, 2} and tables == AC.FUZZ_CASES // 2


# ---- the formatters ---------------------------------------------------------------------------------------------------------------------
def _result():
    case = AC.block_case([AC.blk(0, 100, 0, 1000), AC.blk(0, 150, 0, 968, 1), AC.blk(0, 400, 1, 50), AC.blk(1, 0, 1, 500)], [1000, 300], [5000, 900],
                         [(0, 0, 300, 0), (0, 300, 1000, 1), (1, 0, 300, 0)], [0, 2, 3])
    return restated(case)


def test_assess_row_against_a_literal():
    from ntjoin_amd.report import ASSESS_COLUMNS, assess_row
    assert ASSESS_COLUMNS == ("query reference query_records query_bases reference_bases anchors blocks chains aligned_query_bases "
                              "covered_reference_bases chained_reference_bases NA50 LA50 NGA50 LGA50 NGA75 LGA75 NGA90 LGA90 NG50 LG50 "
                              "translocations_join translocations_contig inversions_join inversions_contig relocations_join relocations_contig").split()
    # four chains of 82 bases: aligned 328 of 1300 (na: 50 % = 650 out of reach), subject 5900: out of reach too; ng: 1000, 1300 < 2950
    # breakpoints: 0|1 inversion at a turning anchor inside piece 0 (contig); 1|2 translocation, 231 in piece 0, 400 in piece 1 (join)
    row = assess_row("scaf.fa", "ref.fa", 2, 9, _result())
    assert row == "scaf.fa\tref.fa\t2\t1300\t5900\t9\t4\t4\t328\t278\t328\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t1\t0\t0\t1\t0\t0"


def test_breakpoint_lines_against_literals():
    from ntjoin_amd.report import breakpoint_lines
    lines = breakpoint_lines(_result(), ["ntJoin0", "tig:0-300"], "ref.fa", ["chr1", "chr2"])
    assert lines == ["ntJoin0\t150\t182\tinversion|contig\tref.fa\tchr1+\tchr1-\n", "ntJoin0\t232\t400\ttranslocation|join\tref.fa\tchr1-\tchr2+\n"]
    # q_lo == q_hi: the interval is one base wide
    touching = A.assess([AC.blk(0, 100, 0, 1000), AC.blk(0, 182, 0, 500)], 32, [1000], [5000])
    assert breakpoint_lines(touching, ["s"], "r", ["c"]) == ["s\t182\t183\trelocation|contig\tr\tc+\tc+\n"]


# ---- the surface ----------------------------------------------------------------------------------------------------------------------
def test_symbol_and_layouts():
    import ctypes as C

    from ntjoin_amd import capi
    header = open(os.path.join(REPO, "include", "ntjoin_mx.h"), encoding="utf-8").read()
    assert "mxg_synteny_assess" in capi.SYMBOLS and re.search(r"\bint mxg_synteny_assess\(", header)
    assert C.sizeof(capi.AssessParams) == 16 and C.sizeof(capi.AssessView) == 376 and C.sizeof(capi.Nx) == 48
    api = open(os.path.join(CSRC, "api.cpp"), encoding="utf-8").read()
    assert "sizeof(mxg_assess_params) == 16" in api and "sizeof(mxg_assess_view) == 376" in api
    assert (capi.BP_TRANSLOCATION, capi.BP_INVERSION, capi.BP_RELOCATION) == (A.TRANSLOCATION, A.INVERSION, A.RELOCATION) == (0, 1, 2)
    assert capi.ASSESS_CHAIN_FIELDS == A.CHAIN_FIELDS and capi.ASSESS_BP_FIELDS == A.BP_FIELDS


def test_command_line_flags():
    from ntjoin_amd.run import parse_arguments
    argv = ["-s", "t.fa.k32.w100.tsv", "-r", "1", "-k", "32", "r.fa.k32.w100.tsv"]
    off = parse_arguments(argv)
    assert off.assess is False and (off.assess_merge_gap, off.assess_max_indel, off.assess_join_indel) == (100000, 1000, 100000)
    on = parse_arguments(argv + ["--assess", "--assess_merge_gap", "0", "--assess_max_indel", "50", "--assess_join_indel", "7"])
    assert on.assess is True and (on.assess_merge_gap, on.assess_max_indel, on.assess_join_indel) == (0, 50, 7) and on.synteny is False


def test_print_scaffolds_refuses_blocks_parameters_that_differ():
    "synteny= and assess= share the scaffolds' blocks call: differing max_gap / min_anchors / min_span are refused before any work"
    from ntjoin_amd.ntjoin import Ntjoin
    nt = Ntjoin.__new__(Ntjoin)   # (the refusal comes before the object is looked at)
    for syn, asz in ((dict(max_gap=5), True), (True, dict(min_anchors=2, merge_gap=0)), (dict(min_span=1), dict(min_span=2))):
        with pytest.raises(ValueError, match="must agree"):
            nt.print_scaffolds([], synteny=syn, assess=asz)
    with pytest.raises(AttributeError):   # the same parameters, spelled or defaulted, pass the check (and reach the missing engine)
        nt.print_scaffolds([], synteny=dict(max_gap=100000), assess=dict(min_anchors=3, max_indel=7))


def test_make_front_end_hands_the_flags_on():
    def dry(*extra):
        res = subprocess.run([os.path.join(REPO, "ntJoin-mx"), "-n", "scaffold", "target=t.fa", "references=r.fa", "reference_weights=2"] + list(extra),
                             capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        return res.stdout
    plain, on = dry(), dry("assess=True")
    flags = " --assess --assess_merge_gap 100000 --assess_max_indel 1000 --assess_join_indel 100000"
    assert "--assess" not in plain and on.replace(flags + " --synteny_max_gap 100000 --synteny_min_anchors 3", "") == plain
    both = dry("assess=True", "synteny=True", "assess_max_indel=5", "synteny_max_gap=0")
    assert " --synteny --synteny_max_gap 0 --synteny_min_anchors 3 --assess --assess_merge_gap 100000 --assess_max_indel 5 --assess_join_indel 100000 " in both
    assert both.count("--synteny_max_gap") == 1
