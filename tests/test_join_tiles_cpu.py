"""CPU test of the size rule for level 1's tiles per thread block (ntjoin_amd/csrc/join_plan.h: pj1_tiles, pj1_launch_tiles,
pj_tiles_grid): a small host program compiled against the header answers for tile counts and for whole plans.  Expected values
come from the rule as join_plan.h states it -- one tile per block below PJ1_TILES_G2 tiles per launch (a threshold no real launch reaches, as measured), two from
there on or where forced, on the 12-byte route only, per launch -- and from the sizes worked out here (an assembly of n minimizers is ceil(ceil(n / 256) / 16)
tiles of 4096)."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import REPO

CSRC = os.path.join(REPO, "ntjoin_amd", "csrc")
INCLUDE = os.path.join(REPO, "include")

PROGRAM = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include "join_plan.h"
using namespace mxg;
static bool rd(uint64_t &v) { return scanf("%" SCNu64, &v) == 1; }
static uint64_t get() { uint64_t v = 0; if (!rd(v)) exit(2); return v; }
static void put(uint64_t v) { printf("%" PRIu64 " ", v); }
int main()
{
    uint64_t cmd;
    while (rd(cmd)) {
        if (cmd == 0) {  // the threshold
            put(PJ1_TILES_G2);
        } else if (cmd == 1) {  // rule: tiles rec12 forced -> G, grid
            const uint64_t tiles = get();
            const bool rec12 = get() != 0;
            const uint32_t forced = (uint32_t)get();
            const uint32_t g = pj1_tiles(tiles, rec12, forced);
            put(g); put(pj_tiles_grid(tiles, g));
        } else {  // plan: split forced A n[A] -> two_level rec12, then G of every launch (split: one per assembly; else the one launch)
            JoinRequest rq;
            JoinLearnt l;
            rq.split = get() != 0;
            rq.pj_tiles = (uint32_t)get();
            rq.A = (uint32_t)get();
            for (uint32_t a = 0; a < rq.A; ++a) rq.n_of[a] = get();
            JoinShape s;
            if (join_shape(rq, l, s) != JS_OK) exit(3);
            put(s.two_level && s.pj); put(s.rec12);
            if (s.split) for (uint32_t a = 0; a < s.A; ++a) put(pj1_launch_tiles(s, a, a + 1));
            else put(pj1_launch_tiles(s, 0, s.A));
        }
        printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    d = tmp_path_factory.mktemp("join_tiles")
    src, exe = d / "join_tiles.cpp", d / "join_tiles"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-I", INCLUDE, str(src), "-o", str(exe)])

    def go(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        rows = [list(map(int, ln.split())) for ln in out.splitlines()]
        assert len(rows) == len(lines)
        return rows
    return go


def tiles_of(n):
    return -(-(-(-n // 256)) // 16)


def by_size(tiles, thr):
    return 2 if tiles >= thr else 1


def test_one_tile_below_the_threshold(run):
    """G = 1 below the threshold; as measured no launch of a real size reaches it (1 465 tiles at 3 Gbp + 3 Gbp, 2^18 tiles at the
    2^30 minimizers the stage takes at most)"""
    (thr,), = run(["0"])
    assert thr > 1 << 18
    counts = [0, 1, 2, 511, 512, 1465, 4395, 1 << 18, thr - 1, thr]
    rows = run([f"1 {t} 1 0" for t in counts])
    for t, (g, grid) in zip(counts, rows):
        assert g == by_size(t, thr), t
        assert grid == -(-t // g), t
    assert [r[0] for r in rows[:8]] == [1] * 8


def test_monotone_in_the_tile_count(run):
    counts = list(range(0, 3000, 7)) + [1 << 20, 1 << 31, (1 << 32) - 1, 1 << 32]
    gs = [r[0] for r in run([f"1 {t} 1 0" for t in counts])]
    assert gs == sorted(gs) and set(gs) <= {1, 2}


def test_forced_values(run):
    cases = [(t, f) for t in (1, 100, 5000) for f in (0, 1, 2, 3, 4, 8)]
    rows = run([f"1 {t} 1 {f}" for t, f in cases])
    (thr,), = run(["0"])
    for (t, f), (g, grid) in zip(cases, rows):
        assert g == (f if f in (1, 2) else by_size(t, thr)), (t, f)   # widths that are not built are not forced
        assert grid == -(-t // g)


def test_16_byte_route_keeps_one_tile(run):
    rows = run([f"1 {t} 0 {f}" for t in (1, 5000) for f in (0, 1, 2)])
    assert all(g == 1 for g, _ in rows)


def test_rule_is_taken_per_launch(run):
    """the fused call's layout (sub-ranges: a launch per assembly): every launch is asked with ITS tile count -- by size each of
    these answers 1 -- and a forced width goes to every launch of the 12-byte route, small or large"""
    (thr,), = run(["0"])
    big, small = 6_000_000, 400_000
    rows = run([f"2 1 0 3 {big} {small} {big}", f"2 1 0 2 {small} {big}", f"2 1 2 3 {big} {small} {big}", f"2 1 1 2 {big} {big}",
                f"2 0 0 2 {big} {big}", f"2 0 2 2 {big} {big}"])
    g = lambda n: by_size(tiles_of(n), thr)  # noqa: E731
    assert rows[0] == [1, 1, g(big), g(small), g(big)] == [1, 1, 1, 1, 1]
    assert rows[1] == [1, 1, g(small), g(big)]
    assert rows[2] == [1, 1, 2, 2, 2]
    assert rows[3] == [1, 1, 1, 1]
    assert rows[4] == [1, 0, 1] and rows[5] == [1, 0, 1]   # one launch for all assemblies, 16-byte records: one tile, forced or not
