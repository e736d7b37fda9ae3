"""CPU test of the host's verdict on a sketch batch (ntjoin_amd/csrc/batch_ctrl.h): a small host program compiled against the
header evaluates BatchReport::ended_well and the report's accessors on a table of reports."""
import os
import shutil
import subprocess

from tests.conftest import REPO

CSRC = os.path.join(REPO, "ntjoin_amd", "csrc")
UNSET = 0xFFFFFFFF
# report words (batch_ctrl.h: ReportWord)
ARENA_NEED, STRETCHES, SELECTED, REDO, CAND, STRETCH_MX, TOTAL, OUT_BASE, GAP_KMERS, DEFERRED, SLICE_GAVE_UP, SEL_REQS = \
    0, 1, 2, 3, 4, 5, 6, 8, 10, 11, 12, 15

PROGRAM = r"""
#include <cstdio>
#include "batch_ctrl.h"
int main()
{
    uint32_t w[mxg::REPORT_WORDS];
    unsigned dev, deferred_ok, empty_ok;
    for (;;) {
        for (uint32_t i = 0; i < mxg::REPORT_WORDS; ++i)
            if (scanf("%u", &w[i]) != 1) return 0;
        if (scanf("%u %u %u", &dev, &deferred_ok, &empty_ok) != 3) return 1;
        const mxg::BatchReport r{w};
        printf("%d %d %llu %llu %u %u %u\n", (int)r.ended_well(dev, deferred_ok, empty_ok), (int)r.reported(),
               (unsigned long long)r.total(), (unsigned long long)r.out_base(), r.gap_kmers(), r.n_deferred(), r.sel_requests());
    }
}
"""


def report(**words):
    """a report that ended the common way (one batch with candidates, no stretch), with `words` changed"""
    w = [0] * 16
    w[SELECTED], w[CAND], w[TOTAL], w[OUT_BASE] = 900, 9000, 900, 100
    for name, v in words.items():
        w[globals()[name.upper()]] = v
    return w


def early_report(arena_need, stretches):
    """what k_emit reports for an arena overflow or a batch without candidates: two words, the rest 0"""
    w = [0] * 16
    w[ARENA_NEED], w[STRETCHES] = arena_need, stretches
    return w


# (case, report, dev_route, deferred_ok, empty_ok, expected verdict)
CASES = [
    ("common way", report(), 0, 0, 0, True),
    ("common way, every allowance of the caller given", report(), 1, 1, 1, True),
    ("unset sentinel", [UNSET] * 16, 1, 1, 1, False),
    ("arena overflow", early_report(5000, 0), 1, 1, 1, False),
    ("arena overflow, stretches seen", early_report(5000, 12), 1, 1, 1, False),
    ("flag: the host must redo", report(redo=1), 1, 1, 1, False),
    ("slice gave up", report(slice_gave_up=1), 1, 1, 1, False),
    ("stretches, not the device route", report(stretches=3, stretch_mx=40), 0, 1, 0, False),
    ("stretches, device route", report(stretches=3, stretch_mx=40), 1, 0, 0, True),
    ("deferred stretches, acceptable to the caller", report(stretches=3, deferred=2), 1, 1, 0, True),
    ("deferred stretches, the counts already used", report(stretches=3, deferred=2), 1, 0, 0, False),
    ("deferred stretches, not the device route", report(stretches=3, deferred=2), 0, 1, 0, False),
    ("no candidates, candidate-array route", early_report(0, 0), 0, 1, 0, False),
    ("no candidates, candidate-array route, device route", early_report(0, 4), 1, 1, 0, False),
    ("no candidates, slice-kernel route", report(cand=0, selected=0, total=0), 0, 1, 1, True),
    ("no candidates, slice-kernel route: contigs as stretches", report(cand=0, selected=0, total=0, stretches=2), 1, 1, 1, True),
    ("no candidates, slice-kernel route, stretches not on the device", report(cand=0, stretches=2), 0, 1, 1, False),
]


def _run(lines, tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    src, exe = tmp_path / "verdict.cpp", tmp_path / "verdict"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    return [list(map(int, l.split())) for l in out.splitlines()]


def test_ended_well_on_a_table_of_reports(tmp_path):
    lines = [" ".join(map(str, w + [dev, dok, eok])) for _, w, dev, dok, eok, _ in CASES]
    got = _run(lines, tmp_path)
    assert len(got) == len(CASES)
    for (name, _, _, _, _, want), row in zip(CASES, got):
        assert bool(row[0]) == want, name


def test_report_accessors(tmp_path):
    w = report(total=7, out_base=3, gap_kmers=11, deferred=2, sel_reqs=5)
    w[TOTAL + 1], w[OUT_BASE + 1] = 1, 2
    got = _run([" ".join(map(str, w + [1, 1, 0])), " ".join(map(str, [UNSET] * 16 + [1, 1, 0]))], tmp_path)
    assert got[0][1:] == [1, 7 + (1 << 32), 3 + (2 << 32), 11, 2, 5]
    reported, gap_kmers, deferred, sel_reqs = got[1][1], *got[1][4:]
    assert (reported, gap_kmers, deferred, sel_reqs) == (0, 0, 0, 0)  # (counts a batch may leave unset read as 0)
