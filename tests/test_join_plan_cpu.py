"""CPU test of the graph stage's join arithmetic (ntjoin_amd/csrc/join_plan.h): a small host program compiled against the header
evaluates join_shape, join_overflow_verdict and JoinLearnt's members on tables of cases.  Every expected value is worked out by
hand from the rules of plan_join / build_graph_impl (the derivation stands beside it), none by running the header.

One rule cannot be shown deciding anything: "n_max >= 2^29 drops the LDS join".  An assembly of 2^29 minimizers means P1 = 4096
coarse partitions, and the two-level join already ends where P1 * 256 * (PJ_T + 1) reaches 2^29, i.e. beyond P1 = 512
(131 072 000 minimizers).  The case is pinned all the same (the join is dropped), next to that limit itself."""
import os
import shutil
import subprocess

from tests.conftest import REPO

CSRC = os.path.join(REPO, "ntjoin_amd", "csrc")
INCLUDE = os.path.join(REPO, "include")
FULL, DG_VERTICES, DG_EDGES, DG_EDGES_APPLIED = 0, 1, 2, 3
RETRY_GLOBAL, RETRY_PJ = 1, 2
LIMIT = 0xFFFFF000  # = 1048575 * 4096: a coarse partition's records are counted in 32 bits

PROGRAM = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include "join_plan.h"
using namespace mxg;
static bool rd(uint64_t &v) { return scanf("%" SCNu64, &v) == 1; }
static uint64_t get() { uint64_t v = 0; if (!rd(v)) exit(2); return v; }
static void put(uint64_t v) { printf("%" PRIu64 " ", v); }
static void get_learnt(JoinLearnt &l, uint32_t n)
{
    l.overflowed = get(); l.cap1_P1 = (uint32_t)get(); l.cap1_need = get(); l.sig = get(); l.sub_P1 = (uint32_t)get(); l.dg_off = get();
    for (uint32_t a = 0; a < n; ++a) l.sub_need[a] = get();
}
static void put_learnt(const JoinLearnt &l, uint32_t n)
{
    put(l.overflowed); put(l.cap1_P1); put(l.cap1_need); put(l.sig); put(l.sub_P1); put(l.dg_off);
    for (uint32_t a = 0; a < n; ++a) put(l.sub_need[a]);
}
int main()
{
    uint64_t cmd;
    while (rd(cmd)) {
        JoinLearnt l;
        if (cmd == 0) {  // shape: A mode bounds global split force2 join_global | learnt | n_of[A]
            JoinRequest rq;
            rq.A = (uint32_t)get(); rq.mode = (int)get(); rq.bounds = get(); rq.global_table = get(); rq.split = get();
            rq.force_two_level = get(); rq.join_global = get();
            get_learnt(l, rq.A);
            for (uint32_t a = 0; a < rq.A; ++a) rq.n_of[a] = get();
            JoinShape s;
            put(join_shape(rq, l, s));
            put(s.cap); put(s.mask); put(s.full); put(s.P); put(s.P1); put(s.cap1); put(s.rows2); put(s.two_level); put(s.pj); put(s.dg_pj);
            put(s.split); put(s.n_sub); put(s.nb); put(s.nb0); put(s.nvs); put(s.n_items); put(s.e_blocks); put(s.n_cur);
            for (uint32_t a = 0; a < rq.A; ++a) { put(s.sub_off[a]); put(s.sub_cap[a]); put(s.skew_lim[a]); }
            for (uint32_t a = 0; a <= rq.A; ++a) put(s.bstart[a]);
        } else if (cmd == 1) {  // verdict: split P1 n_sub cap1 sub_cap[n_sub] | learnt | cursors[P1 * n_sub]
            JoinShape s;
            s.split = get(); s.P1 = (uint32_t)get(); s.n_sub = (uint32_t)get(); s.cap1 = (uint32_t)get();
            for (uint32_t a = 0; a < s.n_sub; ++a) s.sub_cap[a] = (uint32_t)get();
            get_learnt(l, s.n_sub);
            static uint32_t cur[64 * PJ1_CS];
            for (uint32_t i = 0; i < s.P1 * s.n_sub; ++i) {
                for (uint32_t j = 1; j < PJ1_CS; ++j) cur[i * PJ1_CS + j] = 0xFFFFFFFFu;  // (only the first word of a line is a cursor)
                cur[i * PJ1_CS] = (uint32_t)get();
            }
            put(join_overflow_verdict(s, cur, l));
            put_learnt(l, s.n_sub);
        } else {  // learnt: n | learnt | op (0: sketches_are(sig), 1: assembly_added, 2: gave_up) sig
            const uint32_t n = (uint32_t)get();
            get_learnt(l, n);
            const uint64_t op = get(), sig = get();
            if (op == 0) l.sketches_are(sig);
            else if (op == 1) l.assembly_added();
            else l.gave_up();
            put_learnt(l, n);
        }
        printf("\n");
    }
    uint64_t two[2] = {1000, 3000}, one[1] = {5};
    put(JoinLearnt::signature(2, two)); put(JoinLearnt::signature(1, one));
    printf("\n");
    return 0;
}
"""


def _run(lines, tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    src, exe = tmp_path / "join_plan.cpp", tmp_path / "join_plan"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-I", INCLUDE, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    return [list(map(int, l.split())) for l in out.splitlines()]


def learnt(n, overflowed=0, cap1_P1=0, cap1_need=0, sig=0, sub_P1=0, dg_off=0, sub_need=None):
    return [overflowed, cap1_P1, cap1_need, sig, sub_P1, dg_off] + list(sub_need or [0] * n)


SHAPE_FIELDS = ["err", "cap", "mask", "full", "P", "P1", "cap1", "rows2", "two_level", "pj", "dg_pj", "split", "n_sub", "nb", "nb0", "nvs",
                "n_items", "e_blocks", "n_cur"]


def shape(n_of, mode=FULL, bounds=0, global_table=0, split=0, force2=0, join_global=0, **lr):
    A = len(n_of)
    return " ".join(map(str, [0, A, mode, bounds, global_table, split, force2, join_global] + learnt(A, **lr) + list(n_of)))


def parse_shape(row, A):
    d = dict(zip(SHAPE_FIELDS, row))
    rest = row[len(SHAPE_FIELDS):]
    d["sub"] = [tuple(rest[3 * a:3 * a + 3]) for a in range(A)]  # (offset, capacity, skew limit) per assembly
    d["bstart"] = rest[3 * A:]
    return d


SMALL = [1000, 3000]  # 4000 minimizers: P = 256 (256 * 1280 >= 4000), global table of 8192 slots (>= 2 * 4000), 4 + 12 blocks of 256

# (name, input line, A, expected fields)
SHAPE_CASES = [
    # 4096 * 1280 = 5 242 880 minimizers fill PJ_MAX_P partitions of 1280 exactly: one level.  Table: 2^24 >= 2 N > 2^23.
    ("one level at PJ_MAX_P * 1280", shape([2621440, 2621440]), 2,
     dict(err=0, cap=1 << 24, mask=(1 << 24) - 1, full=3, P=4096, P1=0, cap1=0, rows2=0, two_level=0, pj=1, dg_pj=0, split=0, n_sub=1,
          nb=20480, nb0=10240, nvs=2621440, n_items=5242880, e_blocks=20480, n_cur=0, bstart=[0, 10240, 20480])),
    # one more: P would be 8192.  P1: 16 * 256 000 < N <= 32 * 256 000.  Mean 163 840; + 25 % + 4096 = 208 896 = 51 * 4096.
    ("two levels one minimizer beyond", shape([2621440, 2621441]), 2,
     dict(err=0, P=256, P1=32, cap1=208896, rows2=51, two_level=1, pj=1, split=0, n_sub=1, nb=20481, nb0=10240, nvs=2621440,
          n_items=5242880, e_blocks=20480, n_cur=0, sub=[(0, 208896, 0), (0, 0, 0)], bstart=[0, 10240, 20481])),
    ("small input: one level, no coarse partitions", shape(SMALL), 2,
     dict(err=0, cap=8192, mask=8191, full=3, P=256, P1=0, cap1=0, rows2=0, two_level=0, pj=1, nb=16, nb0=4, nvs=1000, n_items=2000,
          e_blocks=8, bstart=[0, 4, 16])),
    # forced: P1 = 2 (2 * 256 000 >= 4000).  Mean 2000; 2000 + 500 + 4096 = 6596 -> 8192.
    ("forced two levels", shape(SMALL, force2=1), 2, dict(err=0, P=256, P1=2, cap1=8192, rows2=2, two_level=1, pj=1, n_cur=0)),
    ("learnt need, same P1", shape(SMALL, force2=1, cap1_P1=2, cap1_need=10000), 2, dict(cap1=12288, rows2=3, two_level=1, pj=1)),
    ("learnt need below the default", shape(SMALL, force2=1, cap1_P1=2, cap1_need=5000), 2, dict(cap1=8192, rows2=2)),
    ("learnt need, other P1", shape(SMALL, force2=1, cap1_P1=4, cap1_need=10000), 2, dict(cap1=8192, rows2=2)),
    ("learnt sub-range need does not size the unsplit layout", shape(SMALL, force2=1, sub_P1=2, sub_need=[9000, 9000]), 2, dict(cap1=8192)),
    # split: means 500 and 1500; 500 + 125 + 4096 = 4721 -> 8192, 1500 + 375 + 4096 = 5971 -> 8192; skew limits 500 + 15 + 2048
    # and 1500 + 46 + 2048; cursors: P1 * A * 32 words
    ("split", shape(SMALL, force2=1, split=1), 2,
     dict(err=0, P1=2, cap1=16384, rows2=4, two_level=1, pj=1, split=1, n_sub=2, n_cur=128, sub=[(0, 8192, 2563), (8192, 8192, 3594)])),
    ("split, learnt need of one assembly", shape(SMALL, force2=1, split=1, sub_P1=2, sub_need=[0, 9000]), 2,
     dict(cap1=20480, rows2=5, two_level=1, sub=[(0, 8192, 2563), (8192, 12288, 3594)])),
    ("split, learnt need for other P1", shape(SMALL, force2=1, split=1, sub_P1=4, sub_need=[0, 9000]), 2, dict(cap1=16384, rows2=4)),
    ("split, learnt whole-partition need does not size sub-ranges", shape(SMALL, force2=1, split=1, cap1_P1=2, cap1_need=99999), 2,
     dict(cap1=16384)),
    ("split asked for, one level: no sub-ranges", shape(SMALL, split=1), 2, dict(P1=0, split=0, n_sub=1, n_cur=0, pj=1)),
    ("split without the LDS join: no cursors among the counts", shape(SMALL, force2=1, split=1, global_table=1), 2,
     dict(split=1, two_level=1, pj=0, n_cur=0)),
    # saturation: a need of LIMIT + 1 rounds up to 2^32; offset and capacity stop at LIMIT, the two-level join is off, and with it pj
    ("split, capacities saturate", shape(SMALL, force2=1, split=1, sub_P1=2, sub_need=[LIMIT + 1, 0]), 2,
     dict(err=0, cap1=LIMIT, rows2=1048575, two_level=0, pj=0, n_cur=0, sub=[(0, LIMIT, 2563), (LIMIT, 8192, 3594)])),
    # what drops the LDS join
    ("global table requested", shape(SMALL, global_table=1), 2, dict(pj=0, two_level=0)),
    ("MXG_GRAPH_JOIN=global", shape(SMALL, join_global=1), 2, dict(pj=0)),
    ("mode: owner's second half", shape(SMALL, mode=DG_EDGES), 2, dict(pj=0, dg_pj=0)),
    ("mode: owner's second half, adjacency applied", shape(SMALL, mode=DG_EDGES_APPLIED), 2, dict(pj=0, dg_pj=0)),
    ("mode: owner's vertices over sections", shape(SMALL, mode=DG_VERTICES), 2, dict(pj=0, dg_pj=0)),
    ("mode: owner's vertices over slots", shape(SMALL, mode=DG_VERTICES, bounds=1), 2, dict(pj=1, dg_pj=1)),
    ("mode: owner's vertices over slots, failed once", shape(SMALL, mode=DG_VERTICES, bounds=1, dg_off=1), 2, dict(pj=0, dg_pj=0)),
    ("bounds alone change nothing", shape(SMALL, bounds=1), 2, dict(pj=1, dg_pj=0)),
    # the two-level join's own limit: P1 = 512 is the last with P1 * 256 * 2049 < 2^29.  512 * 256 000 = 131 072 000: mean 256 000,
    # + 64 000 + 4096 = 324 096 -> 80 * 4096; table 2^28 >= 262 144 000
    ("largest two-level join", shape([65536000, 65536000]), 2,
     dict(err=0, cap=1 << 28, P=256, P1=512, cap1=327680, rows2=80, two_level=1, pj=1, nb=512000, nvs=65536000, n_items=131072000,
          e_blocks=512000)),
    # ... one more: P1 = 1024, mean 128 000, + 32 000 + 4096 = 164 096 -> 41 * 4096
    ("beyond it: global table", shape([65536000, 65536001]), 2, dict(err=0, P1=1024, cap1=167936, rows2=41, two_level=0, pj=0)),
    # an assembly of 2^29: N = 536 871 912, P1 = 4096 (2048 * 256 000 < N), mean 131 072, + 32 768 + 4096 = 167 936 = 41 * 4096
    ("n_max = 2^29", shape([1 << 29, 1000]), 2, dict(err=0, P=256, P1=4096, cap1=167936, rows2=41, two_level=0, pj=0, nvs=1000)),
    ("2^30 minimizers", shape([1 << 29, 1 << 29]), 2, dict(err=1)),
    ("32 assemblies", shape([300] * 32), 32, dict(err=0, full=0xFFFFFFFF, nb=64, nb0=2, nvs=300, n_items=9600, e_blocks=38, pj=1)),
    ("an empty assembly", shape([0, 3000]), 2, dict(err=0, nvs=0, n_items=0, e_blocks=0, nb=12, nb0=0, bstart=[0, 0, 12], pj=1)),
]


def test_shape_on_a_table_of_sizes(tmp_path):
    got = _run([line for _, line, _, _ in SHAPE_CASES], tmp_path)
    assert len(got) == len(SHAPE_CASES) + 1
    for (name, _, A, want), row in zip(SHAPE_CASES, got):
        d = parse_shape(row, A)
        for key, v in want.items():
            assert d[key] == v, (name, key, d[key], v)


def verdict(split, P1, sub_cap, cursors, **lr):
    """cursors[c][s]: what coarse partition c's sub-range s counted"""
    n_sub = len(sub_cap)
    flat = [x for row in cursors for x in row]
    assert len(cursors) == P1 and len(flat) == P1 * n_sub
    return " ".join(map(str, [1, split, P1, n_sub, sum(sub_cap)] + list(sub_cap) + learnt(n_sub, **lr) + flat))


# (name, input line, n_sub, verdict, learnt afterwards: cap1_P1, cap1_need, sub_P1, sub_need)
VERDICT_CASES = [
    # one cursor per coarse partition, capacity 8192
    ("nothing overflowed (a table did): global", verdict(0, 2, [8192], [[5000], [6000]]), 1, RETRY_GLOBAL, (0, 0, 0, [0])),
    ("full to the brim is no overflow", verdict(0, 2, [8192], [[8192], [6000]]), 1, RETRY_GLOBAL, (0, 0, 0, [0])),
    # 9000 + 9000 / 8 + 4096 = 14 221
    ("a partition overflowed: re-size", verdict(0, 2, [8192], [[5000], [9000]]), 1, RETRY_PJ, (2, 14221, 0, [0])),
    ("learnt for another P1: re-size", verdict(0, 2, [8192], [[5000], [9000]], cap1_P1=4, cap1_need=99999), 1, RETRY_PJ, (2, 14221, 0, [0])),
    ("learnt less than this: re-size", verdict(0, 2, [8192], [[5000], [9000]], cap1_P1=2, cap1_need=8999), 1, RETRY_PJ, (2, 14221, 0, [0])),
    ("already learnt: global, no loop", verdict(0, 2, [8192], [[5000], [9000]], cap1_P1=2, cap1_need=14221), 1, RETRY_GLOBAL,
     (2, 14221, 0, [0])),
    ("already learnt exactly this count: global", verdict(0, 2, [8192], [[5000], [9000]], cap1_P1=2, cap1_need=9000), 1, RETRY_GLOBAL,
     (2, 9000, 0, [0])),
    # a sub-range per assembly, 8192 each.  Partition totals 12 000 and 6000: 12 000 + 1500 + 4096 = 17 596 for the one-cursor layout
    ("split, nothing overflowed: global; P1 recorded, needs cleared", verdict(1, 2, [8192, 8192], [[3000, 8000], [2000, 4000]], sub_P1=4,
                                                                            sub_need=[7, 7]), 2, RETRY_GLOBAL, (0, 0, 2, [0, 0])),
    ("split, one sub-range overflowed: re-size", verdict(1, 2, [8192, 8192], [[3000, 9000], [2000, 4000]]), 2, RETRY_PJ,
     (2, 17596, 2, [0, 14221])),
    ("split, the sum would fit but a sub-range does not", verdict(1, 2, [8192, 8192], [[100, 9000], [100, 100]]), 2, RETRY_PJ,
     (2, 9100 + 9100 // 8 + 4096, 2, [0, 14221])),
    ("split, a larger whole-partition need is kept", verdict(1, 2, [8192, 8192], [[3000, 9000], [2000, 4000]], cap1_P1=2, cap1_need=50000),
     2, RETRY_PJ, (2, 50000, 2, [0, 14221])),
    ("split, whole-partition need of another P1 is dropped", verdict(1, 2, [8192, 8192], [[3000, 9000], [2000, 4000]], cap1_P1=4,
                                                                   cap1_need=50000), 2, RETRY_PJ, (2, 17596, 2, [0, 14221])),
    ("split, already learnt: global, no loop", verdict(1, 2, [8192, 8192], [[3000, 9000], [2000, 4000]], cap1_P1=2, cap1_need=17596, sub_P1=2,
                                                     sub_need=[0, 14221]), 2, RETRY_GLOBAL, (2, 17596, 2, [0, 14221])),
]


def test_verdict_on_cursor_tables(tmp_path):
    got = _run([line for _, line, _, _, _ in VERDICT_CASES], tmp_path)
    for (name, _, n_sub, want, (cap1_P1, cap1_need, sub_P1, sub_need)), row in zip(VERDICT_CASES, got):
        assert row[0] == want, (name, row)
        overflowed, g_P1, g_need, _, g_sub_P1, dg_off = row[1:7]
        assert (overflowed, dg_off) == (0, 0), name  # (the verdict leaves them to build_graph and the owner)
        assert (g_P1, g_need, g_sub_P1, row[7:7 + n_sub]) == (cap1_P1, cap1_need, sub_P1, sub_need), (name, row)


def test_what_the_handle_forgets(tmp_path):
    everything = dict(overflowed=1, cap1_P1=2, cap1_need=5, sig=111, sub_P1=2, dg_off=1, sub_need=[3, 4])
    only_sub = dict(sig=111, sub_P1=2, sub_need=[3, 4])
    lines = [" ".join(map(str, [2, 2] + learnt(2, **l) + [op, sig]))
             for l, op, sig in [(everything, 0, 111), (everything, 0, 222), (only_sub, 0, 222), (everything, 1, 0), ({}, 2, 0)]]
    got = _run(lines, tmp_path)
    # the same sketches: nothing forgotten
    assert got[0] == [1, 2, 5, 111, 2, 1, 3, 4]
    # other sketches: the global-table mark, the whole-partition need and the sub-ranges' P1 go; sub_need[] and dg_off stay
    assert got[1] == [0, 0, 0, 222, 0, 1, 3, 4]
    # ... but only if the handle overflowed or learnt a whole-partition need: sub-range needs alone are kept
    assert got[2] == [0, 0, 0, 222, 2, 0, 3, 4]
    # an assembly added: the sub-ranges' needs, the signature and dg_off stay
    assert got[3] == [0, 0, 0, 111, 2, 1, 3, 4]
    assert got[4] == [1, 0, 0, 0, 0, 0, 0, 0]
    # signature: 0x9E3779B97F4A7C15 * (assemblies + 1), then (s ^ n) * 0x100000001B3 per assembly, mod 2^64
    M = (1 << 64) - 1
    s2 = (0x9E3779B97F4A7C15 * 3) & M
    for n in (1000, 3000):
        s2 = ((s2 ^ n) * 0x100000001B3) & M
    assert s2 == 16364723682650144183
    assert got[5] == [16364723682650144183, 5007962544327997405]
