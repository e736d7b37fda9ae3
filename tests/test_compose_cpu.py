"""CPU tests of the composition of piece tables (include/ntjoin_mx.h, row f11): the code of the device route
(ntjoin_amd/csrc/compose.h) run serially on the host by tools/compose_check.cpp, built plainly and with AddressSanitizer +
UndefinedBehaviorSanitizer (the runtime linked into the program; nothing is preloaded), against the restatement of the contract
(tests/_compose_restatement.py) on the hand-made cases, a seeded fuzz and the refusals of tests/_compose_cases.py; in every case a
record spells the same sequence before and after; the exported symbol and the layout the Python side mirrors."""
import os
import shutil
import subprocess

import pytest

from tests import _compose_cases as cases, _compose_restatement as R
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
    td = tmp_path_factory.mktemp("compose_check_" + request.param)
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    extra = []
    if request.param == "sanitized":
        extra = _sanitizer_flags(cxx, td)
        if extra is None:
            pytest.skip("the host compiler has no AddressSanitizer runtime to link")
    out = td / "compose_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror"] + extra +
                          ["-I", os.path.join(REPO, "include"), "-I", CSRC, os.path.join(REPO, "tools", "compose_check.cpp"), "-o", str(out)])
    return str(out)


def _table_text(table):
    return " ".join([str(len(table))] + [" ".join([str(len(rec))] + [" ".join(map(str, p)) for p in rec]) for rec in table])


def _run(exe, inner, outer, tmp_path):
    f = tmp_path / "tables.txt"
    f.write_text(_table_text(inner) + "\n" + _table_text(outer) + "\n")
    return subprocess.run([exe, str(f)], capture_output=True, text=True, timeout=120)


def _parse(stdout):
    result = []
    for line in stdout.splitlines():
        v = [int(x) for x in line.split()]
        assert len(v) == 1 + 4 * v[0]
        result.append([tuple(v[1 + 4 * j:5 + 4 * j]) for j in range(v[0])])
    return result


def test_restatement_on_a_case_worked_by_hand():
    "the issue's own example: an outer cut inside an inner gap next to an outer gap gives one gap"
    F, V, G = R.FWD, R.REV, R.GAP
    got = R.compose(cases.HAND["cut_in_gap_next_to_outer_gap"][:2], cases.INNER)
    assert got[0] == [(1, 0, 50, F), (0, 0, 30, G), (2, 100, 160, V), (0, 0, 5, G), (3, 7, 47, F)]
    assert got[1] == [(3, 7, 47, V), (0, 0, 5, G), (2, 100, 160, F), (0, 0, 30, G), (1, 0, 50, V)]
    assert R.compose([[(1, 80, 120, V)]], cases.INNER) == [[(2, 110, 150, F)]]   # REV over REV, clipped at both ends


@pytest.mark.parametrize("name", sorted(cases.HAND))
def test_hand_made_cases(exe, name, tmp_path):
    outer = cases.HAND[name]
    want = R.compose(outer, cases.INNER)
    cases.check_spelling(cases.BASE_LEN, cases.INNER, outer, want)
    r = _run(exe, cases.INNER, outer, tmp_path)
    assert r.returncode == 0, r.stderr
    assert _parse(r.stdout) == want


def test_seeded_fuzz(exe, tmp_path):
    for seed in range(120):
        base_len, inner, outer = cases.fuzz_case(seed, inner_pieces=(None, 1, 37)[seed % 3], outer_pieces=(4, 1, 12)[seed % 3])
        want = R.compose(outer, inner)
        cases.check_spelling(base_len, inner, outer, want, seed)
        r = _run(exe, inner, outer, tmp_path)
        assert r.returncode == 0, (seed, r.stderr)
        assert _parse(r.stdout) == want, seed


def test_composition_is_associative(exe, tmp_path):
    "three rounds: composing round 3 with (round 2 over round 1) equals composing (round 3 over round 2) with round 1"
    for seed in range(20):
        base_len, t1, t2 = cases.fuzz_case(seed)
        rng = cases.random.Random(1000 + seed)
        t3 = cases.random_table(rng, 3, [R.record_length(rec) for rec in t2])
        assert R.compose(t3, R.compose(t2, t1)) == R.compose(R.compose(t3, t2), t1), seed
        r = _run(exe, R.compose(t2, t1), t3, tmp_path)
        assert r.returncode == 0 and _parse(r.stdout) == R.compose(R.compose(t3, t2), t1), seed


@pytest.mark.parametrize("name", sorted(cases.REFUSED))
def test_refusals(exe, name, tmp_path):
    inner, outer, code = cases.REFUSED[name]
    with pytest.raises(R.Refused) as ei:
        R.compose(outer, inner)
    assert ei.value.code == code
    r = _run(exe, inner, outer, tmp_path)
    assert r.returncode == {R.EINVAL: 3, R.ELIMIT: 4}[code] and r.stderr.strip() and not r.stdout


def test_symbol_constants_and_layout():
    import numpy as np
    from ntjoin_amd import capi
    from ntjoin_amd.engine import MxEngine
    assert "mxg_compose_pieces" in capi.SYMBOLS
    assert (capi.PIECE_FWD, capi.PIECE_REV, capi.PIECE_GAP) == (R.FWD, R.REV, R.GAP)
    assert MxEngine.SEQ_PIECE.itemsize == 16 and MxEngine.SEQ_PIECE.names == ("record", "start", "end", "kind")
    header = open(os.path.join(REPO, "include", "ntjoin_mx.h"), encoding="utf-8").read()
    for name, value in (("MXG_PIECE_FWD", R.FWD), ("MXG_PIECE_REV", R.REV), ("MXG_PIECE_GAP", R.GAP)):
        assert f"#define {name} {value}u" in header
    assert np.dtype(MxEngine.SEQ_PIECE).fields["kind"][1] == 12
