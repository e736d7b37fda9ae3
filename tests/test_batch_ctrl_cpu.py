"""CPU test of the host's verdict on a sketch batch (ntjoin_amd/csrc/batch_ctrl.h): a small host program compiled against the
header evaluates BatchReport::ended_well and the report's accessors on a table of reports, and the header's pure launch
arithmetic (gap_placing, grid_by_estimate) and its two layouts of SC_CTRL on tables whose expected values are written out by hand."""
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


def _run(lines, tmp_path, program=PROGRAM):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    src, exe = tmp_path / "verdict.cpp", tmp_path / "verdict"
    src.write_text(program)
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


# ---- the launch arithmetic and the layouts of SC_CTRL: one line per case, its first word says which function
ARITHMETIC = r"""
#include <cstdio>
#include "batch_ctrl.h"
int main()
{
    char what;
    while (scanf(" %c", &what) == 1) {
        if (what == 'P') {  // gcap gap_rate nk rate_hint forced
            unsigned gcap; double rate, hint; unsigned long long nk, forced;
            if (scanf("%u %lf %llu %lf %llu", &gcap, &rate, &nk, &hint, &forced) != 5) return 1;
            const mxg::GapPlacing p = mxg::gap_placing(gcap, rate, nk, hint, forced);
            printf("%u %lld %u\n", p.n_place, (long long)(p.gap_expect * 1000.0), p.place4);
        } else if (what == 'G') {  // knob nk tau_hi min_variant hint n_cap rk tile
            unsigned long long knob, nk, hint; unsigned tau_hi, minv, n_cap, rk, tile;
            if (scanf("%llu %llu %u %u %llu %u %u %u", &knob, &nk, &tau_hi, &minv, &hint, &n_cap, &rk, &tile) != 8) return 1;
            printf("%u\n", mxg::grid_by_estimate(knob, nk, tau_hi, minv != 0, hint, n_cap, rk, tile));
        } else if (what == 'C') {  // words of the two super-count arrays
            unsigned a, b;
            if (scanf("%u %u", &a, &b) != 2) return 1;
            const mxg::CandCtrlLayout l = mxg::cand_ctrl_layout(a, b);
            printf("%u %u %u %zu\n", l.wave_sup, l.sel_sup, l.words, l.bytes());
        } else if (what == 'S') {  // words of the slices' super-counts
            unsigned a;
            if (scanf("%u", &a) != 1) return 1;
            const mxg::SliceCtrlLayout l = mxg::slice_ctrl_layout(a);
            printf("%u %u %u %u %zu\n", l.sup, l.cand_spread, l.tickets, l.words, l.bytes());
        } else {
            return 1;
        }
    }
    return 0;
}
"""

GCAP = 4096
R20 = 2.0 ** -20  # a stretch rate that is exact in binary: R20 * (n << 20) stretches are exactly n
# (case, gcap, gap_rate, nk, rate_hint, forced) -> (n_place, gap_expect in thousandths, place4)
PLACING = [
    ("no hint yet: blocks for all the arrays hold, nothing expected", (GCAP, R20, 100 << 20, 0.0, 0), (1024, -1000, 4096)),
    ("hint, 2 * 100 + 256 = 456 < gcap", (GCAP, R20, 100 << 20, 1e-6, 0), (114, 100000, 456)),
    ("hint, 2 * 100.5 + 256 = 457: rounded up to whole blocks", (GCAP, R20, 201 << 19, 1e-6, 0), (115, 100500, 460)),
    ("hint, 2 * 4000 + 256 > gcap", (GCAP, R20, 4000 << 20, 1e-6, 0), (1024, 4000000, 4096)),
    ("forced 8 < gcap", (GCAP, R20, 100 << 20, 0.0, 8), (2, -1000, 8)),
    ("forced 9: three blocks, and the hint's expectation is dropped", (GCAP, R20, 100 << 20, 1e-6, 9), (3, -1000, 12)),
    ("forced 10000 > gcap", (GCAP, R20, 100 << 20, 1e-6, 10000), (1024, -1000, 4096)),
]
RK, TILE = 256, 16 * 256
TAU10 = 1 << 22  # tau_hi / 2^32 = 2^-10: 102400000 k-mers make 100000 candidates expected
# (case, knob, nk, tau_hi, min_variant, hint, n_cap) -> candidates the grids cover
GRID = [
    ("knob 0: the capacity", (0, 102400000, TAU10, 0, 0, 10000000), 0),
    ("100000 * 1.3 + 16384 = 146384 -> 36 tiles", (1, 102400000, TAU10, 0, 0, 10000000), 147456),
    ("hint 200000 > expect: 276384 -> 68 tiles", (1, 102400000, TAU10, 0, 200000, 10000000), 278528),
    ("hint below expect changes nothing", (1, 102400000, TAU10, 0, 5000, 10000000), 147456),
    ("test value 2: 400 / 2 < RK -> RK -> one tile", (2, 409600, TAU10, 0, 0, 100000), 4096),
    ("test value 2: 100000 / 2 -> 13 tiles, the hint ignored", (2, 102400000, TAU10, 0, 200000, 10000000), 53248),
    ("capped by the capacity", (1, 102400000, TAU10, 0, 0, 100000), 100000),
    ("min variant: 200000 expected, 276384 -> 68 tiles", (1, 102400000, TAU10, 1, 0, 10000000), 278528),
    ("40960 * 1.3 + 16384 = 17 tiles exactly: not rounded further", (1, 1024000, TAU10, 0, 40960, 10000000), 69632),
]
# sup_words (scan_kernels.h: 32 words per 256 producer blocks begun, and one more) of 1 block, and of 256: 32 and 64 words
SUP_1, SUP_256 = 32, 64
# candidate-array route (words of wave_sup, words of sel_sup) -> (wave_sup, sel_sup, words, bytes)
CAND_LAYOUT = [
    ("one wave, two k_resolve blocks", (SUP_1, SUP_1), (16, 48, 80, 320)),
    ("256 waves, 256 k_resolve blocks", (SUP_256, SUP_256), (16, 80, 144, 576)),
    ("one wave, 256 k_resolve blocks", (SUP_1, SUP_256), (16, 48, 112, 448)),
]
# slice route (words of the slices' super-counts) -> (sup, cand_spread, tickets, words, bytes)
SLICE_LAYOUT = [
    ("one slice", SUP_1, (16, 48, 2096, 4144, 16576)),
    ("256 slices", SUP_256, (16, 80, 2128, 4176, 16704)),
]


def test_gap_placing_on_a_table(tmp_path):
    got = _run(["P " + " ".join(repr(v) for v in args) for _, args, _ in PLACING], tmp_path, ARITHMETIC)
    assert len(got) == len(PLACING)
    for (name, _, want), row in zip(PLACING, got):
        assert tuple(row) == want, name
        assert row[2] == 4 * row[0], name  # (Item::place4)


def test_grid_by_estimate_on_a_table(tmp_path):
    got = _run(["G " + " ".join(map(str, args + (RK, TILE))) for _, args, _ in GRID], tmp_path, ARITHMETIC)
    assert len(got) == len(GRID)
    for (name, args, want), row in zip(GRID, got):
        assert row == [want], name
        assert want % TILE == 0 or want == args[5], name  # (whole k_emit tiles, or the capacity)


def test_ctrl_layouts_on_a_table(tmp_path):
    lines = ["C %d %d" % args for _, args, _ in CAND_LAYOUT] + ["S %d" % sup for _, sup, _ in SLICE_LAYOUT]
    got = _run(lines, tmp_path, ARITHMETIC)
    assert len(got) == len(lines)
    for (name, _, want), row in zip(CAND_LAYOUT, got):
        assert tuple(row) == want, name
    for (name, sup, want), row in zip(SLICE_LAYOUT, got[len(CAND_LAYOUT):]):
        assert tuple(row) == want, name
        # the size the slice route's fill has always had: control words, super-counts, two rows of 64 counters 32 words apart
        assert row[3] == 16 + sup + 2 * 64 * 32 and row[4] == 4 * row[3], name
