"""CPU test of the rank predicate of the graph stage's edge passes (ntjoin_amd/csrc/graph_rank.h): "v is next to u in assembly b"
decided from the places of u and v in b's filtered list and the records of those places, the support mask of a pair and the
"first supporter" rule.  A small host program compiled against the header answers for every item (a, r) of hand-made filtered
lists; what it must answer comes from a brute-force neighbour list built here (consecutive entries of one record are neighbours),
i.e. from the definition the adjacency table of k_adjacency implements, not from ranks."""
import os
import shutil
import subprocess

import numpy as np

from tests.conftest import REPO

CSRC = os.path.join(REPO, "ntjoin_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "graph_rank.h"
using namespace mxg;
int main()
{
    unsigned A, nv;
    while (scanf("%u %u", &A, &nv) == 2) {
        std::vector<std::vector<uint32_t>> fv(A, std::vector<uint32_t>(nv)), frec(fv), rank(fv);
        for (unsigned a = 0; a < A; ++a) {
            for (unsigned r = 0; r < nv; ++r)
                if (scanf("%u", &fv[a][r]) != 1) return 2;
            for (unsigned r = 0; r < nv; ++r)
                if (scanf("%u", &frec[a][r]) != 1) return 2;
            for (unsigned r = 0; r < nv; ++r) rank[a][fv[a][r]] = r;
        }
        auto rank_of = [&](uint32_t b, uint32_t x) { return b ? rank[b][x] : x; };  // assembly 0: the vertex id is the place
        auto rec_at = [&](uint32_t b, uint32_t r) { return frec[b][r]; };
        for (unsigned a = 0; a < A; ++a)
            for (unsigned r = 0; r < nv; ++r) {
                const bool succ = r + 1 < nv && frec[a][r + 1] == frec[a][r];
                if (!succ) {
                    printf("%u %u 0 0 0 0\n", a, r);
                    continue;
                }
                const uint32_t u = fv[a][r], v = fv[a][r + 1];
                const uint32_t m = rank_support_mask(A, u, v, rank_of, rec_at);
                // the same mask, pair by pair, the way the kernels' fast path asks: rank_fetch + the two records
                uint32_t m2 = 0;
                for (unsigned b = 0; b < A; ++b) {
                    uint32_t lo, hi;
                    const bool w = rank_fetch(true, rank_of(b, u), rank_of(b, v), nv, lo, hi);
                    if (lo >= nv && nv) return 3;
                    if (hi >= nv && nv) return 3;
                    if (!w && (lo || hi)) return 4;
                    if (w && hi != lo + 1) return 5;
                    if (w && frec[b][lo] == frec[b][hi]) m2 |= 1u << b;
                    if (rank_neighbours(rank_of(b, u), rank_of(b, v), frec[b][rank_of(b, u)], frec[b][rank_of(b, v)]) != ((m >> b) & 1u)) return 6;
                }
                printf("%u %u 1 %u %u %u\n", a, r, m, m2, (unsigned)rank_edge_flag(m, a, A));
            }
        printf("end\n");
    }
    // not wanted, out of the row, not adjacent: place 0 twice and "do not compare"
    uint32_t lo = 9, hi = 9;
    if (rank_fetch(false, 3, 4, 10, lo, hi) || lo || hi) return 7;
    if (rank_fetch(true, 9, 10, 10, lo, hi) || lo || hi) return 8;
    if (rank_fetch(true, 0xFFFFFFFFu, 0, 10, lo, hi) || lo || hi) return 9;
    if (rank_fetch(true, 3, 5, 10, lo, hi) || lo || hi) return 10;
    if (rank_fetch(true, 4, 4, 10, lo, hi) || lo || hi) return 11;
    if (!rank_fetch(true, 9, 8, 10, lo, hi) || lo != 8 || hi != 9) return 12;
    if (rank_first_supporter(0, 0) || !rank_first_supporter(6, 1) || rank_first_supporter(6, 2)) return 13;
    // a run of items is unused iff no item of it lies below the count of its row: against the loop over the items
    for (uint32_t stride : {1u, 2u, 5u, 8u})
        for (uint32_t rows = 1; rows <= 3; ++rows)
            for (uint32_t count = 0; count <= stride; ++count)
                for (uint32_t first = 0; first <= rows * stride + 2; ++first)
                    for (uint32_t n = 0; n <= 2 * stride + 2; ++n) {
                        bool used = false;
                        for (uint32_t i = first; i < first + n && i < rows * stride; ++i) used |= i % stride < count;
                        if (rank_items_unused(first, n, rows * stride, stride, count) == used) return 14;
                    }
    if (!rank_items_unused(0xFFFFFF00u, 1024u, 0xFFFFFFF0u, 0x7FFFFFF8u, 5u)) return 15;  // (first + n beyond 2^32)
    if (rank_items_unused(0x7FFFFFF0u, 1024u, 0xFFFFFFF0u, 0x7FFFFFF8u, 5u)) return 16;   // (reaches the next row)
    return 0;
}
"""


def _case(lists):
    """lists[a] = records of assembly a, each a list of vertex ids; assembly 0 must list 0, 1, 2, ... in order"""
    fv = [np.array([v for rec in recs for v in rec], dtype=np.int64) for recs in lists]
    frec = [np.array([i for i, rec in enumerate(recs) for _ in rec], dtype=np.int64) for recs in lists]
    nv = fv[0].size
    assert np.array_equal(fv[0], np.arange(nv))
    for f in fv:
        assert sorted(f.tolist()) == list(range(nv)), "every vertex once in every assembly"
    return fv, frec


def _brute(fv, frec):
    """per item (a, r): (has successor, support mask, flag byte) from neighbour sets"""
    A, nv = len(fv), fv[0].size
    nbr = []
    for a in range(A):
        s = set()
        for r in range(nv - 1):
            if frec[a][r] == frec[a][r + 1]:
                s.add((int(fv[a][r]), int(fv[a][r + 1])))
                s.add((int(fv[a][r + 1]), int(fv[a][r])))
        nbr.append(s)
    rows = []
    for a in range(A):
        for r in range(nv):
            if r + 1 >= nv or frec[a][r] != frec[a][r + 1]:
                rows.append((a, r, 0, 0, 0, 0))
                continue
            u, v = int(fv[a][r]), int(fv[a][r + 1])
            m = sum(1 << b for b in range(A) if (u, v) in nbr[b])
            first = min(b for b in range(A) if m >> b & 1) == a
            flag = 0 if not first else (m if A <= 8 else 1)
            rows.append((a, r, 1, m, m, flag))
    return rows


def _random_case(A, nv, seed):
    rng = np.random.default_rng(seed)
    lists = []
    for a in range(A):
        order = list(range(nv))
        if a:
            # records of assembly 0 kept, reversed or shuffled, so that many pairs stay neighbours
            cut = sorted(set(rng.integers(1, nv, size=nv // 5).tolist()))
            chunks = [order[i:j] for i, j in zip([0] + cut, cut + [nv])]
            rng.shuffle(chunks)
            order = []
            for ch in chunks:
                how = rng.integers(0, 3)
                order += ch if how == 0 else ch[::-1] if how == 1 else rng.permutation(ch).tolist()
        cut = sorted(set(rng.integers(1, nv, size=max(nv // 7, 1)).tolist()))
        lists.append([order[i:j] for i, j in zip([0] + cut, cut + [nv])])
    return lists


CASES = {
    "one assembly, three records": [[[0, 1, 2], [3], [4, 5]]],
    # (1, 2) adjacent in assembly 1 in reverse order; 3 and 4 sit at neighbouring places of assembly 1 in different records: no
    # support; [6] is a record of one vertex; 7 ends both rows
    "two assemblies by hand": [[[0, 1, 2, 3, 4, 5], [6], [7]], [[2, 1, 0], [5, 3], [4, 6, 7]]],
    "one vertex": [[[0]], [[0]]],
    "two vertices, two records": [[[0], [1]], [[1, 0]]],
    "A3": _random_case(3, 60, 1),
    "A4": _random_case(4, 60, 2),
    "A5": _random_case(5, 40, 3),
    "A8": _random_case(8, 40, 4),
    "A9": _random_case(9, 40, 5),  # beyond eight the flag byte only says "edge"
    "A32": _random_case(32, 30, 6),
}


def test_rank_predicate_equals_brute_force_neighbours(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    src, exe = tmp_path / "graph_rank.cpp", tmp_path / "graph_rank"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    text, want = [], []
    for name, lists in CASES.items():
        fv, frec = _case(lists)
        text.append(f"{len(fv)} {fv[0].size}")
        for a in range(len(fv)):
            text.append(" ".join(map(str, fv[a].tolist())))
            text.append(" ".join(map(str, frec[a].tolist())))
        want.append(_brute(fv, frec))
    out = subprocess.run([str(exe)], input="\n".join(text) + "\n", capture_output=True, text=True, check=True).stdout
    blocks = [b.strip().splitlines() for b in out.split("end\n") if b.strip()]
    assert len(blocks) == len(CASES)
    for (name, _), rows, ref in zip(CASES.items(), blocks, want):
        got = [tuple(map(int, ln.split())) for ln in rows]
        assert got == ref, name
    # the hand case, spelt out: items of assembly 0 then of assembly 1 as (successor, mask, flag)
    hand = _brute(*_case(CASES["two assemblies by hand"]))
    by = {(a, r): (s, m, f) for a, r, s, m, _, f in hand}
    assert by[(0, 0)] == (1, 3, 3) and by[(0, 1)] == (1, 3, 3), "(0,1) and (1,2): adjacent in assembly 1 in reverse order"
    assert by[(0, 3)] == (1, 1, 1), "3 and 4: neighbouring places of assembly 1, different records"
    assert by[(0, 5)] == (0, 0, 0) and by[(0, 6)] == (0, 0, 0) and by[(0, 7)] == (0, 0, 0)
    assert by[(1, 0)] == (1, 3, 0) and by[(1, 1)] == (1, 3, 0), "assembly 0 supports them first"
    assert by[(1, 3)] == (1, 2, 2), "(5, 3): assembly 1 alone"
    assert by[(1, 5)] == (1, 2, 2) and by[(1, 6)] == (1, 2, 2) and by[(1, 7)] == (0, 0, 0)
