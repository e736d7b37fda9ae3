"""CPU test of the size rule of the graph stage's ordered passes (graph_tail_u / graph_tail_grid in ntjoin_amd/csrc/join_plan.h):
how many 256-blocks a thread block takes, and that the grid made from it covers every block.  A small host program compiled
against the header prints the values; what they must be follows from the rule's own statement (1 below GRAPH_TAIL_U2 blocks, 4
from GRAPH_TAIL_U4 on, never 0, never narrower for more blocks), not from running it."""
import os
import shutil
import subprocess

from tests.conftest import REPO

CSRC = os.path.join(REPO, "ntjoin_amd", "csrc")
INCLUDE = os.path.join(REPO, "include")

PROGRAM = r"""
#include <cinttypes>
#include <cstdio>
#include "join_plan.h"
using namespace mxg;
int main()
{
    printf("%u %u %u\n", GRAPH_TAIL_U2, GRAPH_TAIL_U4, GRAPH_TAIL_U_VERTICES);
    uint64_t blocks, forced;
    while (scanf("%" SCNu64 " %" SCNu64, &blocks, &forced) == 2) {
        const uint32_t U = graph_tail_u(blocks, (uint32_t)forced);
        printf("%u %u\n", U, graph_tail_grid(blocks, U));
    }
    // the plan carries the rule's answers: flag pass by nb, edge passes by e_blocks, the knob forces all of them
    for (uint32_t forced : {0u, 1u, 2u, 4u, 3u}) {
        JoinRequest rq;
        rq.A = 2;
        rq.n_of[0] = rq.n_of[1] = (uint64_t)GRAPH_TAIL_U4 * 256;  // nb = 2 * GRAPH_TAIL_U4, e_blocks = 2 * GRAPH_TAIL_U4
        rq.graph_u = forced;
        JoinShape s;
        JoinLearnt l;
        const int rc = join_shape(rq, l, s);
        printf("%d %u %u %u %u %u\n", rc, s.nb, s.e_blocks, s.u_flags, s.u_vertices, s.u_edges);
    }
    {
        JoinRequest rq;
        rq.A = 2;
        rq.n_of[0] = 1000;
        rq.n_of[1] = (uint64_t)GRAPH_TAIL_U4 * 256;  // many minimizers, few vertices: the edge passes stay narrow
        JoinShape s;
        JoinLearnt l;
        const int rc = join_shape(rq, l, s);
        printf("%d %u %u %u %u %u\n", rc, s.nb, s.e_blocks, s.u_flags, s.u_vertices, s.u_edges);
    }
    return 0;
}
"""


def _run(pairs, tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    src, exe = tmp_path / "tail_plan.cpp", tmp_path / "tail_plan"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-I", INCLUDE, str(src), "-o", str(exe)])
    text = "".join(f"{b} {f}\n" for b, f in pairs)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout
    rows = [list(map(int, l.split())) for l in out.splitlines()]
    return rows[0], rows[1:1 + len(pairs)], rows[1 + len(pairs):]


MAX_BLOCKS = 2**32 // 256 - 1  # the most 256-blocks a pass can have: its items are counted in 32 bits


def test_width_by_size_is_1_2_4_monotone_and_never_0(tmp_path):
    (u2, u4, uv), _, _ = _run([], tmp_path)
    assert 0 < u2 < u4 and uv in (1, 2, 4)
    sizes = sorted({0, 1, 2, 255, 256, u2 - 1, u2, u2 + 1, (u2 + u4) // 2, u4 - 1, u4, u4 + 1, 46_700, 1 << 20, MAX_BLOCKS})
    _, rows, _ = _run([(b, 0) for b in sizes], tmp_path)
    widths = [r[0] for r in rows]
    assert all(w in (1, 2, 4) for w in widths)
    assert widths == sorted(widths), "more blocks, never a narrower pass"
    by = dict(zip(sizes, widths))
    assert by[0] == by[1] == by[u2 - 1] == 1, "below the small threshold: one 256-block per thread block"
    assert by[u2] == by[u4 - 1] == 2
    assert by[u4] == by[46_700] == by[MAX_BLOCKS] == 4, "from the large threshold on (the headline's 46 700 blocks): four"


def test_knob_forces_1_2_4_and_nothing_else(tmp_path):
    sizes = (0, 1, 5000, 1 << 20)
    _, rows, _ = _run([(b, f) for f in (1, 2, 4) for b in sizes], tmp_path)
    assert [r[0] for r in rows] == [f for f in (1, 2, 4) for _ in sizes]
    _, rows, _ = _run([(b, f) for f in (3, 5, 8, 2**32 - 1) for b in sizes], tmp_path)
    _, by_size, _ = _run([(b, 0) for b in sizes], tmp_path)
    assert [r[0] for r in rows] == [r[0] for r in by_size] * 4, "not a width: as if the knob were not set"


def test_grid_covers_every_block(tmp_path):
    cases = []
    for u in (1, 2, 4):
        for blocks in (0, 1, u - 1, u, u + 1, MAX_BLOCKS):
            cases.append((blocks, u))
    _, rows, _ = _run(cases, tmp_path)
    for (blocks, u), (got_u, grid) in zip(cases, rows):
        assert got_u == u
        assert grid * u >= blocks, "a block beyond the grid"
        assert grid == 0 or (grid - 1) * u < blocks, "a thread block with nothing to do"
        assert grid == -(-blocks // u)
        assert grid < 2**31


def test_plan_carries_the_widths(tmp_path):
    (u2, u4, uv), _, plans = _run([], tmp_path)
    nb = 2 * u4
    want = {0: (4, min(4, uv), 4), 1: (1, 1, 1), 2: (2, 2, 2), 4: (4, 4, 4), 3: (4, min(4, uv), 4)}
    for forced, row in zip((0, 1, 2, 4, 3), plans):
        assert row[0] == 0 and row[1] == nb and row[2] == nb
        assert tuple(row[3:]) == want[forced], forced
    # 1000 + 4 194 304 minimizers: nb = 4 + u4 blocks of minimizers, 2 * 1000 items = 8 blocks of edges
    rc, nb2, eb2, uf, uvx, ue = plans[5]
    assert (rc, nb2, eb2) == (0, 4 + u4, 8)
    assert (uf, uvx, ue) == (4, min(4, uv), 1)
