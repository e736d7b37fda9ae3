"""CPU test of the two-level join's 12-byte records and of the learnt verdict prefill (ntjoin_amd/csrc/join_plan.h,
join_verdict.h): a small host program compiled against the headers packs, unpacks and compares records and asks join_shape and
JoinLearnt for their choices.  Every expected value is worked out here from the rule, none by running the header:

  product = key * 0x9E3779B97F4A7C15 mod 2^64; coarse partition = bits 52 .. 52 + lg P1 - 1, fine partition = bits 44 .. 44 + lg P - 1.
  Those bits are implied by where a level-2 record lies.  The 6-bit tag (assembly | mark << 5) replaces the lowest six of them,
  the fine partition's first.  Two records of one fine partition have equal keys iff their words agree outside the tag."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import REPO

CSRC = os.path.join(REPO, "ntjoin_amd", "csrc")
INCLUDE = os.path.join(REPO, "include")
MUL = 0x9E3779B97F4A7C15
INV = pow(MUL, -1, 1 << 64)
ONES = (1 << 64) - 1

PROGRAM = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include "join_plan.h"
#include "join_verdict.h"
using namespace mxg;
static bool rd(uint64_t &v) { return scanf("%" SCNu64, &v) == 1; }
static uint64_t get() { uint64_t v = 0; if (!rd(v)) exit(2); return v; }
static void put(uint64_t v) { printf("%" PRIu64 " ", v); }
int main()
{
    uint64_t cmd;
    while (rd(cmd)) {
        if (cmd == 0) {  // record: P1 P key assembly dup -> fits coarse fine lo word tag key12
            const uint32_t P1 = (uint32_t)get(), P = (uint32_t)get();
            const uint64_t key = get(), prod = key * PJ_MUL;
            const uint32_t a = (uint32_t)get();
            const bool dup = get() != 0;
            const uint32_t lgP = pj12_lg(P);
            const uint32_t word = pj12_pack((uint32_t)(prod >> 32), lgP, pj12_tag(a, dup));
            put(pj12_fits(P1, P)); put(pj12_coarse(prod, P1)); put(pj12_fine(prod, P)); put((uint32_t)prod); put(word);
            put(pj12_unpack_tag(word, lgP)); put(pj12_key((uint32_t)prod, word, lgP));
        } else if (cmd == 1) {  // same key?  P keyA aA dupA keyB aB dupB
            const uint32_t lgP = pj12_lg((uint32_t)get());
            uint32_t lo[2], w[2];
            for (int i = 0; i < 2; ++i) {
                const uint64_t prod = get() * PJ_MUL;
                const uint32_t a = (uint32_t)get();
                const bool dup = get() != 0;
                lo[i] = (uint32_t)prod;
                w[i] = pj12_pack((uint32_t)(prod >> 32), lgP, pj12_tag(a, dup));
            }
            put(pj12_same_key(lo[0], w[0], lo[1], w[1], lgP));
        } else if (cmd == 2) {  // shape: split force2 no_rec12 no_pipe no_prefill0 bounds sub_P1 sub_need pre_known pre_shared0 pre_n0 pre_A pre_bounds pre_n[pre_A] A n[A]
            JoinRequest rq;
            JoinLearnt l;
            rq.split = get(); rq.force_two_level = get(); rq.no_rec12 = get(); rq.no_pipe = get(); rq.no_prefill0 = get(); rq.bounds = get();
            l.sub_P1 = (uint32_t)get();
            const uint64_t need = get();
            for (uint32_t a = 0; a < MXG_MAX_ASSEMBLIES; ++a) l.sub_need[a] = need;
            const bool known = get();
            const uint64_t shared0 = get(), n0 = get();
            uint64_t pre_n[MXG_MAX_ASSEMBLIES];
            const uint32_t pre_A = (uint32_t)get();
            const bool pre_bounds = get();
            for (uint32_t a = 0; a < pre_A; ++a) pre_n[a] = get();
            if (known) l.shared_counted(JoinLearnt::prefill_signature(pre_A, pre_n, pre_bounds), shared0, n0);
            const uint64_t added = get();
            if (added) l.assembly_added();
            rq.A = (uint32_t)get();
            for (uint32_t a = 0; a < rq.A; ++a) rq.n_of[a] = get();
            JoinShape s;
            put(join_shape(rq, l, s));
            put(s.P1); put(s.P); put(s.two_level); put(s.pj); put(s.split); put(s.rows2); put(s.rec12); put(s.prefill0);
        } else if (cmd == 4) {  // a sketch replaced behind a join that gave up: shared0 n0 A n[A] -> overflowed before, after, prefill0 after
            JoinLearnt l;
            const uint64_t shared0 = get(), n0 = get();
            JoinRequest rq;
            rq.force_two_level = true;
            rq.A = (uint32_t)get();
            for (uint32_t a = 0; a < rq.A; ++a) rq.n_of[a] = get();
            l.gave_up();
            l.shared_counted(JoinLearnt::prefill_signature(rq.A, rq.n_of, false), shared0, n0);
            put(l.overflowed);
            l.sketch_replaced();
            rq.global_table = l.overflowed;
            JoinShape s;
            join_shape(rq, l, s);
            put(l.overflowed); put(s.pj); put(s.prefill0);
        } else {  // prefill words: rule a i
            const uint32_t rule = (uint32_t)get(), a = (uint32_t)get(), i = (uint32_t)get();
            put(pj_verdict_prefill(rule, a, i)); put(PJ_VERDICT_PREFILL); put(PJ_VERDICT_REF);
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
    d = tmp_path_factory.mktemp("join_records")
    src, exe = d / "join_records.cpp", d / "join_records"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-I", INCLUDE, str(src), "-o", str(exe)])

    def go(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        rows = [list(map(int, ln.split())) for ln in out.splitlines()]
        assert len(rows) == len(lines)
        return rows
    return go


def lg(x):
    return x.bit_length() - 1


def implied_bits(P1, P):
    """bit numbers of the product that the partitions imply, lowest first: the fine partition's, then the coarse one's"""
    return [44 + t for t in range(lg(P))] + [52 + t for t in range(lg(P1))]


def expect_record(P1, P, key, a, dup):
    prod = (key * MUL) & ONES
    tag_at = implied_bits(P1, P)[:6]
    tag = a | (32 if dup else 0)
    packed = prod
    for t, bit in enumerate(tag_at):
        packed = (packed & ~(1 << bit)) | (((tag >> t) & 1) << bit)
    key12 = prod
    for bit in tag_at:
        key12 &= ~(1 << bit)
    return {"coarse": (prod >> 52) & (P1 - 1), "fine": (prod >> 44) & (P - 1), "lo": prod & 0xFFFFFFFF, "word": packed >> 32, "tag": tag,
            "key12": key12}


def key_of(P1, P, coarse, fine, lo, word):
    """the key a level-2 record stands for, from the record and its place alone"""
    prod = (word << 32) | lo
    for bit in implied_bits(P1, P)[:6]:
        prod &= ~(1 << bit)
    prod |= (fine << 44) | (coarse << 52)   # (implied bits outside the tag are in the word already, and agree)
    return (prod * INV) & ONES


# every (P1, P) join_shape can produce with two levels (P = 256, P1 = 2 .. 4096), the one-level shapes (P1 = 0: no coarse
# partitions, 16 bytes whatever P), and shapes around the condition P1 * P >= 64 that only the helpers see: 2 x 32 and 64 x 1 are
# the smallest that fit, 2 x 16 and 32 x 1 the largest that do not
TWO_LEVEL = [(1 << q, 256) for q in range(1, 13)]
ONE_LEVEL = [(0, 1 << p) for p in range(8, 13)]
EDGE_FIT = [(2, 32), (64, 1), (4, 16), (8, 8), (16, 4)]
EDGE_NOT = [(2, 16), (32, 1), (4, 8), (1, 32)]
KEYS = [0, 1, ONES, 1 << 63, 0x0123456789ABCDEF, (ONES * INV) & ONES, 0xDEADBEEFCAFEF00D]


def test_fits(run):
    shapes = TWO_LEVEL + ONE_LEVEL + EDGE_FIT + EDGE_NOT
    rows = run([f"0 {P1} {P} 5 0 0" for P1, P in shapes])
    for (P1, P), row in zip(shapes, rows):
        assert row[0] == int(P1 != 0 and P1 * P >= 64), (P1, P)
    assert all(P1 * P >= 64 for P1, P in TWO_LEVEL + EDGE_FIT) and all(P1 * P < 64 for P1, P in EDGE_NOT)


@pytest.mark.parametrize("P1,P", TWO_LEVEL + EDGE_FIT)
def test_pack_unpack_and_place_give_the_key_back(P1, P, run):
    cases = [(k, a, d) for k in KEYS for a in (0, 31) for d in (0, 1)]
    rows = run([f"0 {P1} {P} {k} {a} {d}" for k, a, d in cases])
    for (k, a, d), row in zip(cases, rows):
        want = expect_record(P1, P, k, a, d)
        got = dict(zip(("coarse", "fine", "lo", "word", "tag", "key12"), row[1:]))
        assert got == want, (P1, P, hex(k), a, d)
        assert key_of(P1, P, got["coarse"], got["fine"], got["lo"], got["word"]) == k
        assert got["key12"] != ONES  # never the table's empty mark
        assert got["word"] & 0x7FF == (want["key12"] >> 32) & 0x7FF  # the table slot's bits (32..42) lie below the tag


@pytest.mark.parametrize("P1,P", TWO_LEVEL + EDGE_FIT)
def test_equality_rule(P1, P, run):
    """products that differ only in implied bits are different keys in DIFFERENT partitions (their records never meet, and where the
    difference lies in tag bits they compare equal); products that differ in one kept bit -- the lowest, the highest, the one next
    to the tag, the top and the bottom of the word -- share the partition and must compare unequal; the tag never matters"""
    base = 0x0F1E2D3C4B5A6978
    imp = implied_bits(P1, P)
    kept = [b for b in range(64) if b not in imp]
    lines, want = [], []

    def pair(pa, pb, ta, tb, same):
        ka, kb = (pa * INV) & ONES, (pb * INV) & ONES
        lines.append(f"1 {P} {ka} {ta[0]} {ta[1]} {kb} {tb[0]} {tb[1]}")
        want.append(same)

    tags = [(0, 0), (31, 1), (31, 0), (0, 1)]
    for ta in tags:
        for tb in tags:
            pair(base, base, ta, tb, 1)
    for bit in imp[:6]:       # only a tag bit differs: another partition, the same kept bits
        pair(base, base ^ (1 << bit), (0, 0), (0, 0), 1)
        assert (((base ^ (1 << bit)) >> 44) & (P - 1), ((base ^ (1 << bit)) >> 52) & (P1 - 1)) != ((base >> 44) & (P - 1), (base >> 52) & (P1 - 1))
    for bit in imp[6:]:       # an implied bit outside the tag is kept in the word
        pair(base, base ^ (1 << bit), (0, 0), (0, 0), 0)
    for bit in (kept[0], kept[-1], 0, 63 if 63 in kept else kept[-1], 43, 31, 32):
        if bit in kept:
            for ta in ((0, 0), (31, 1)):
                pair(base, base ^ (1 << bit), ta, (0, 0), 0)
    # keys (not products) that differ only in their top or bottom bit
    for kbit in (0, 63):
        ka = 0x1122334455667788
        kb = ka ^ (1 << kbit)
        pa, pb = (ka * MUL) & ONES, (kb * MUL) & ONES
        same_part = ((pa >> 44) & (P - 1), (pa >> 52) & (P1 - 1)) == ((pb >> 44) & (P - 1), (pb >> 52) & (P1 - 1))
        mask = ONES
        for bit in imp[:6]:
            mask &= ~(1 << bit)
        lines.append(f"1 {P} {ka} 0 0 {kb} 31 1")
        want.append(int(pa & mask == pb & mask))
        assert not (same_part and pa & mask == pb & mask)  # the rule: never equal inside one partition
    rows = run(lines)
    assert [r[0] for r in rows] == want


def shape_line(n, split=1, force2=1, no_rec12=0, no_pipe=0, no_prefill0=0, bounds=0, sub_P1=0, sub_need=0, pre=None, added=0):
    """pre = (shared0, n0, sizes, bounds) of the build before"""
    if pre:
        known = [1, pre[0], pre[1], len(pre[2]), pre[3]] + list(pre[2])
    else:
        known = [0, 0, 0, 0, 0]
    return " ".join(map(str, [2, split, force2, no_rec12, no_pipe, no_prefill0, bounds, sub_P1, sub_need] + known + [added, len(n)] + list(n)))


SHAPE = ("err", "P1", "P", "two_level", "pj", "split", "rows2", "rec12", "prefill0")


def test_join_shape_picks_the_record(run):
    big = [6_000_000, 6_000_000]   # 12 M minimizers: P > 4096 -> two levels by itself, P1 = 64 (64 * 256 * 1000 >= 12 M)
    small = [3000, 2500]
    cases = [
        (shape_line(big, force2=0), dict(P1=64, P=256, two_level=1, pj=1, split=1, rec12=1)),
        (shape_line(big, force2=0, split=0), dict(P1=64, two_level=1, split=0, rec12=0)),           # one cursor per partition: 16 bytes
        (shape_line(small), dict(P1=2, P=256, two_level=1, split=1, rows2=4, rec12=1)),             # the smallest two-level shape: 2 x 256
        (shape_line(small, force2=0), dict(P1=0, two_level=0, split=0, rec12=0)),                   # one level
        (shape_line(small, no_rec12=1), dict(P1=2, split=1, rec12=0)),
        (shape_line(small, no_pipe=1), dict(P1=2, split=1, rec12=0)),                               # k_pj_join reads 16 bytes
        # sub-ranges re-sized beyond 256 rows (2 x 602 112 records = 294 rows of 4096): k_pj_join again
        (shape_line(small, sub_P1=2, sub_need=600_000), dict(P1=2, split=1, rows2=294, rec12=0)),
        # ... and just inside: 2 x 524 288 = 256 rows
        (shape_line(small, sub_P1=2, sub_need=524_288), dict(P1=2, split=1, rows2=256, rec12=1)),
    ]
    rows = run([c[0] for c in cases])
    for (line, want), row in zip(cases, rows):
        got = dict(zip(SHAPE, row))
        assert got["err"] == 0
        # (small, two levels: a sub-range holds mean + mean / 4 + 4096 rounded up to 4096 = 8192 records per assembly: 4 rows)
        for key, val in want.items():
            assert got[key] == val, (line, key, got)


def test_learnt_prefill_choice(run):
    n = [1000, 800]
    cases = [
        (shape_line(n), 0),                                                # the first build: nothing known
        (shape_line(n, pre=(490, 1000, n, 0)), 0),                         # 49 %
        (shape_line(n, pre=(500, 1000, n, 0)), 0),                         # 50 %: not more than half
        (shape_line(n, pre=(510, 1000, n, 0)), 1),                         # 51 %
        (shape_line(n, pre=(1000, 1000, n, 0)), 1),
        (shape_line(n, pre=(900, 1000, [1000, 801], 0)), 0),               # other sizes
        (shape_line(n, pre=(900, 1000, [1001, 800], 0)), 0),
        (shape_line(n, pre=(900, 1000, n, 1)), 0),                         # the fused call's bounds are no sizes
        (shape_line(n, bounds=1, pre=(900, 1000, n, 1)), 1),
        (shape_line(n + [700], pre=(900, 1000, n, 0)), 0),                 # an assembly more
        (shape_line(n, pre=(900, 1000, n, 0), added=1), 0),                # assembly_added() forgets
        (shape_line(n, pre=(900, 1000, n, 0), no_prefill0=1), 0),
        (shape_line(n, pre=(900, 1000, n, 0), force2=0), 0),               # one level: k_pj_bucket knows one rule
        (shape_line(n, split=0, pre=(900, 1000, n, 0)), 1),                # two levels without sub-ranges: the rule holds
    ]
    rows = run([c[0] for c in cases])
    for (line, want), row in zip(cases, rows):
        got = dict(zip(SHAPE, row))
        assert got["prefill0"] == want, (line, got)


def test_replaced_sketch_forgets_the_overflow_and_keeps_the_guess(run):
    """sketch_replaced() (mxg_set_sketch_device): the next build tries the LDS join again, with the prefill the build before taught
    -- the guess is keyed by the sizes and stays, right or wrong"""
    assert run(["4 900 1000 2 1000 800", "4 400 1000 2 1000 800"]) == [[1, 0, 1, 1], [1, 0, 1, 0]]


def test_prefill_words_are_distinct(run):
    cases = [(0, 0, 5), (0, 1, 5), (1, 0, 0), (1, 0, 5), (1, 0, (1 << 29) - 1), (1, 1, 5), (1, 31, 0)]
    rows = run([f"3 {r} {a} {i}" for r, a, i in cases])
    for (r, a, i), (word, prefill, refmark) in zip(cases, rows):
        assert (prefill, refmark) == (1, 2)
        assert word == ((i << 3) | 7 if r == 1 and a == 0 else 1), (r, a, i)
        assert word != 0 and word & 7 != refmark  # neither the overflow word nor a reference
