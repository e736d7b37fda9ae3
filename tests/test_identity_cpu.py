"""CPU tests of the identity contract (include/ntjoin_mx.h, row f14): the restatement itself (tests/_identity_restatement.py) on
hand-derived cases, against a full DP wherever it is not saturated, and on the order of the skip rules; then
tools/identity_check.cpp -- the device route's per-segment code (ntjoin_amd/csrc/identity.h) run on the host -- built plainly and
with AddressSanitizer + UndefinedBehaviorSanitizer (the runtime linked into the program; nothing is preloaded), against the
restatement on the hand cases, the boundary shapes and 300 seeded pairs."""
import os
import shutil
import subprocess

import pytest

from tests import _identity_cases as cases, _identity_restatement as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "ntjoin_amd", "csrc")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.HAND, ids=[c[0] for c in cases.HAND])
def test_hand_cases(case):
    _name, q, s, rev, max_seg, expect = case
    assert R.segment(q, s, bool(rev), max_seg) == expect


def test_constants_and_classes():
    assert (R.E, R.MAX_SHIFT, R.DEFAULT_MAX_SEG) == (16, 31, 10000) and R.MAX_SHIFT + 2 * R.E + 1 == 64
    assert [R.byte_class(c) for c in "ACGTUacgtuNn-RYKM*"] == [0, 1, 2, 3, 3, 0, 1, 2, 3, 3] + [4] * 8
    assert R.bases("AC\nGT\r\nA\n") == "ACGTA"
    assert R.classes("AACG", reverse=True) == [1, 2, 3, 3] and R.classes("AN", reverse=True) == [4, 3]


def test_banded_equals_full_unless_saturated():
    "200 seeded mutated pairs: the band's value is the edit distance whenever it is not flagged, and never below it"
    exact = flagged = 0
    for _name, q, s, rev, max_seg in cases.mutated_pairs(200, seed=1, max_len=300):
        edits, status, sat = R.segment(q, s, bool(rev), max_seg)
        if status != R.ALIGNED:
            assert status == R.SKIP_SHIFT and abs(len(q) - len(s)) > R.MAX_SHIFT
            continue
        full = R.full_distance(R.classes(q), R.classes(s, bool(rev)))
        assert sat == (1 if edits > abs(len(q) - len(s)) + 2 * R.E else 0)
        if sat:
            flagged += 1
            assert edits >= full
        else:
            exact += 1
            assert edits == full
    assert exact > 100 and flagged >= 1


def test_band_edge():
    "a detour of E diagonals stays exact; one of E + 1 is forced to the band's edge and flagged"
    by_name = {c[0]: c for c in cases.boundary_cases()}
    for where in ("start", "end", "middle"):
        _n, q, s, rev, m = by_name[f"block16_{where}"]
        assert R.segment(q, s, bool(rev), m) == (32, R.ALIGNED, 0) == (R.full_distance(R.classes(q), R.classes(s)), R.ALIGNED, 0)
        _n, q, s, rev, m = by_name[f"block17_{where}"]
        edits, status, sat = R.segment(q, s, bool(rev), m)
        assert (status, sat) == (R.ALIGNED, 1) and edits > 34 >= R.full_distance(R.classes(q), R.classes(s))
    assert R.segment(*by_name["block16_inserted"][1:]) == (16, R.ALIGNED, 0) and R.segment(*by_name["block17_inserted"][1:]) == (17, R.ALIGNED, 0)
    assert R.segment(*by_name["poly_a_poly_c"][1:]) == (300, R.ALIGNED, 1)


def test_reversed_cases_spell_the_same_pairs():
    fwd = {c[0]: c for c in cases.boundary_cases() if not c[0].endswith("_rev")}
    n = 0
    for name, q, s, rev, m in cases.boundary_cases():
        if name.endswith("_rev"):
            assert rev == 1 and R.segment(q, s, True, m) == R.segment(*fwd[name[:-4]][1:])
            n += 1
    assert n == len(fwd) - 1  # (the palindrome is reversed as it stands)


def test_skip_rules_in_order():
    n, a = "N" * 50, "A" * 6
    assert R.segment(n, a, False, 5) == (0, R.SKIP_LEN, 0)        # too long, shifted and class 4: the length rule
    assert R.segment(a, n, False, 49) == (0, R.SKIP_LEN, 0)       # ... on the subject alone
    assert R.segment(n, a, False, 50) == (0, R.SKIP_SHIFT, 0)     # exactly max_seg: shifted and class 4: the shift rule
    assert R.segment("N" * 37, a, False, 50) == (0, R.SKIP_N, 0)  # |d| = 31: class 4
    assert R.segment("A" * 37, a, False, 50) == (31, R.ALIGNED, 0)
    assert R.segment("ACGT", "ACGT", False, 4) == (0, R.ALIGNED, 0) and R.segment("ACGT", "ACGT", False, 3) == (0, R.SKIP_LEN, 0)


def test_segment_of_records_passes_over_line_ends():
    q, s = ["AC\nGTAC\r\nGT\n"], ["TT\n", "A\nC\nG\nA\nA\nC\n"]
    assert R.segment_of_records(q, s, (0, 1, 5, 1, 1, 5, 0)) == (1, R.ALIGNED, 0)   # CGTAC : CGAAC
    assert R.segment_of_records(q, s, (0, 6, 2, 0, 0, 2, 1)) == (2, R.ALIGNED, 0)   # GT : revcomp(TT) = AA


# ---- tools/identity_check: the device route's code on the host -----------------------------------------------------------------------
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
    td = tmp_path_factory.mktemp("identity_check_" + request.param)
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    extra = []
    if request.param == "sanitized":
        extra = _sanitizer_flags(cxx, td)
        if extra is None:
            pytest.skip("the host compiler has no AddressSanitizer runtime to link")
    out = td / "identity_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror"] + extra +
                          ["-I", os.path.join(REPO, "include"), "-I", CSRC, os.path.join(REPO, "tools", "identity_check.cpp"), "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def restated():
    "the cases the program is run on and what the restatement says of them, computed once for both builds"
    todo = [c[:5] for c in cases.HAND] + cases.boundary_cases() + cases.mutated_pairs(300, seed=2)
    return todo, [R.segment(q, s, bool(rev), m) for _n, q, s, rev, m in todo]


def _run(exe, todo, tmp_path):
    f = tmp_path / "pairs.txt"
    f.write_text("".join(f"{m} {rev} {q} {s}\n" for _n, q, s, rev, m in todo))
    res = subprocess.run([exe, str(f)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    return [tuple(int(x) for x in line.split()) for line in res.stdout.splitlines()]


def test_check_program(exe, restated, tmp_path):
    todo, want = restated
    got = _run(exe, todo, tmp_path)
    assert len(got) == len(want)
    for c, g, w in zip(todo, got, want):
        assert g == w, (c[0], g, w)
    hand = {c[0]: c[5] for c in cases.HAND}
    assert all(g == hand[c[0]] for c, g in zip(todo[:len(cases.HAND)], got))
    pairs = todo[-300:]
    assert min(len(c[1]) for c in pairs) <= 5 and max(len(c[1]) for c in pairs) > 550 and any(c[3] for c in pairs)
    assert {(w[1], w[2]) for w in want} == {(0, 0), (0, 1), (1, 0), (2, 0), (3, 0)}


def test_check_program_refuses_malformed_input(exe, tmp_path):
    for text in ("10 0 ACGT\n", "0 0 ACGT ACGT\n", "x 0 ACGT ACGT\n"):
        f = tmp_path / "bad.txt"
        f.write_text(text)
        assert subprocess.run([exe, str(f)], capture_output=True, timeout=60).returncode == 2
    assert subprocess.run([exe, str(tmp_path / "none.txt")], capture_output=True, timeout=60).returncode == 2
