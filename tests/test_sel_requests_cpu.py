"""CPU test of the request array between k_bs_select and k_sel_stretch at its capacity (ntjoin_amd/csrc/sel_requests.h): a small
host program compiled against the header plays producer and consumer as the kernels do -- slices reserve entries in a random order
into an array that still holds what an earlier batch left, every lane applies sel_req_slot, then the array is walked over
min(counter, capacity) entries with sel_req_is_first -- and reports every entry the walk met that this round did not write.

The same simulation with the rule the kernels had before (a lane writes only if base + n_i <= capacity, else nothing) must FAIL
wherever a reservation straddles the capacity: that is the evidence that this test sees the stale requests k_sel_stretch used to
consume, without a GPU having to read unwritten memory."""
import os
import random
import shutil
import subprocess

import pytest

from tests.conftest import REPO

CSRC = os.path.join(REPO, "ntjoin_amd", "csrc")
NONE, WRITE, TOMBSTONE = 0, 1, 2
SEL_REQ = 8
USABLE = (1 << 18) - 8
NO_KERNEL = 0xFFFFFFFF - SEL_REQ

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "sel_requests.h"
using namespace mxg;
struct Entry { uint32_t w, round; };
// the rule under test, or the one the kernels had before: all of a reservation or none of it, nothing in between
static SelReqSlot rule(int which, uint32_t base, uint32_t n_i, uint32_t lane, uint32_t cap)
{
    if (which == 0) return sel_req_slot(base, n_i, lane, cap);
    return lane < n_i && base + n_i <= cap ? SEL_SLOT_WRITE : SEL_SLOT_NONE;
}
int main()
{
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "consts")) {
            int tomb_first = 0, tomb_number0 = 0;  // over every entry a lane can hold
            for (uint32_t n_i = 1; n_i <= SEL_REQ; ++n_i)
                for (uint32_t q = 0; q < n_i; ++q)
                    for (uint32_t slice : {0u, 1u, 77u, 0xFFFFFFu}) {
                        const uint32_t t = sel_req_tombstone(sel_req_word(slice, q, n_i));
                        tomb_first += sel_req_is_first(t, 1u << 24);
                        tomb_number0 += sel_req_number(t) == 0u;
                    }
            printf("%u %u %u %u %d %d\n", SEL_REQ, SEL_IREQ_USABLE, SEL_IREQ_CAP - SEL_IREQ_USABLE, SEL_REQ_NO_KERNEL, tomb_first, tomb_number0);
        } else if (!strcmp(cmd, "slot")) {
            uint32_t base, n_i, lane, cap;
            if (scanf("%u %u %u %u", &base, &n_i, &lane, &cap) != 4) return 1;
            printf("%u\n", (unsigned)sel_req_slot(base, n_i, lane, cap));
        } else if (!strcmp(cmd, "sim")) {
            // which rule, capacity, what the array held before (0: first requests of in-range slices, 1: of slices no batch has),
            // slices of the batch, then (slice, n_i) in the order the reservations land
            uint32_t which, cap, poison, n_slices, n_arrive;
            if (scanf("%u %u %u %u %u", &which, &cap, &poison, &n_slices, &n_arrive) != 5) return 1;
            std::vector<uint32_t> sl(n_arrive), ni(n_arrive);
            uint64_t total = 0;
            for (uint32_t i = 0; i < n_arrive; ++i) {
                if (scanf("%u %u", &sl[i], &ni[i]) != 2) return 1;
                total += ni[i];
            }
            const uint32_t OLD = 1, NOW = 2;
            std::vector<Entry> arr((size_t)(total > cap ? total : cap) + SEL_IREQ_SPARE);
            for (size_t e = 0; e < arr.size(); ++e)
                arr[e] = Entry{sel_req_word(poison ? 0xFFFFFFu - (uint32_t)(e % 5) : (uint32_t)(e % n_slices), 0u, 1u + (uint32_t)(e % SEL_REQ)), OLD};
            std::vector<uint32_t> written(n_slices, 0), pushed(n_slices, 0), taken(n_slices, 0);
            uint32_t counter = 0, out_of_array = 0;
            for (uint32_t i = 0; i < n_arrive; ++i) {
                const uint32_t base = counter;
                counter += ni[i];  // (the add of lane 0; every lane of the wave then decides for itself)
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    const SelReqSlot s = rule((int)which, base, ni[i], lane, cap);
                    if (s != SEL_SLOT_NONE && base + lane >= cap) ++out_of_array;
                    if (s == SEL_SLOT_WRITE) {
                        arr[base + lane] = Entry{sel_req_word(sl[i], lane, ni[i]), NOW};
                        ++written[sl[i]];
                    } else {
                        if (s == SEL_SLOT_TOMBSTONE) arr[base + lane] = Entry{sel_req_tombstone(sel_req_word(sl[i], lane, ni[i])), NOW};
                        if (lane < ni[i]) ++pushed[sl[i]];
                    }
                }
            }
            // the walk of k_sel_stretch
            uint32_t first_stale = 0, other_stale = 0, beyond = 0;
            const uint32_t n_req = sel_req_walk(counter, cap);
            for (uint32_t r = 0; r < n_req; ++r) {
                const Entry e = arr[r];
                if (!sel_req_is_first(e.w, n_slices)) {
                    if (e.round != NOW) ++other_stale;
                    continue;
                }
                if (e.round != NOW) {
                    ++first_stale;
                    continue;
                }
                const uint32_t n_i = sel_req_count(e.w);
                for (uint32_t q = 0; q < n_i; ++q) {  // lanes q < n_i use what they read at r + q
                    const Entry m = arr[r + q];
                    if (r + q >= cap) ++beyond;
                    else if (m.round != NOW || sel_req_slice(m.w) != sel_req_slice(e.w) || sel_req_number(m.w) != q) ++other_stale;
                }
                ++taken[sel_req_slice(e.w)];
            }
            printf("%u %u %u %u %u", first_stale, other_stale, beyond, out_of_array, n_req);
            for (uint32_t s = 0; s < n_slices; ++s) printf(" %u:%u:%u", written[s], pushed[s], taken[s]);
            printf("\n");
        } else {
            return 1;
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    d = tmp_path_factory.mktemp("sel_requests")
    src, exe = d / "sel_requests.cpp", d / "sel_requests"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])

    def run(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        return out.splitlines()
    return run


def test_constants_and_the_tombstone(program):
    sel_req, usable, spare, no_kernel, tomb_first, tomb_number0 = map(int, program(["consts"])[0].split())
    assert (sel_req, usable, spare, no_kernel) == (SEL_REQ, USABLE, 8, NO_KERNEL)
    assert tomb_first == 0 and tomb_number0 == 0   # (k_sel_stretch steps over an entry whose number in the slice is not 0)


# (base, n_i, lane, capacity) -> what the lane does, derived by hand from the three cases of sel_requests.h
SLOT_TABLE = [
    ((0, 1, 0, 1), WRITE),                    # the only entry of the smallest array
    ((0, 2, 0, 1), TOMBSTONE), ((0, 2, 1, 1), NONE),   # two requests for one entry: the one in front of the capacity is a tombstone
    ((1, 1, 0, 1), NONE),                     # base == capacity: behind the walk
    ((5, 3, 0, 8), WRITE), ((5, 3, 2, 8), WRITE),      # ends exactly at the capacity: fits
    ((5, 4, 0, 8), TOMBSTONE), ((5, 4, 2, 8), TOMBSTONE), ((5, 4, 3, 8), NONE),  # one too many: entries 5, 6, 7 tombstones, 8 is not there
    ((7, 8, 0, 8), TOMBSTONE), ((7, 8, 1, 8), NONE), ((7, 8, 7, 8), NONE),
    ((8, 8, 0, 8), NONE), ((9, 1, 0, 8), NONE),
    ((0, 3, 3, 100), NONE), ((0, 3, 63, 100), NONE), ((0, 0, 0, 100), NONE),     # lanes without a request
    ((0, 8, 7, 100), WRITE), ((92, 8, 7, 100), WRITE), ((93, 8, 6, 100), TOMBSTONE), ((93, 8, 7, 100), NONE),
    # the array as shipped
    ((USABLE - 8, 8, 7, USABLE), WRITE), ((USABLE - 7, 8, 6, USABLE), TOMBSTONE), ((USABLE - 7, 8, 7, USABLE), NONE),
    ((USABLE, 1, 0, USABLE), NONE),
    # sums that would wrap: base + n_i = 4 (mod 2^32) "fits" any capacity -- the rule takes differences
    ((0xFFFFFFFC, 8, 0, 0xFFFFFFFE), TOMBSTONE), ((0xFFFFFFFC, 8, 1, 0xFFFFFFFE), TOMBSTONE), ((0xFFFFFFFC, 8, 2, 0xFFFFFFFE), NONE),
    ((0xFFFFFFFF, 8, 0, 5), NONE), ((0xFFFFFFFF, 1, 0, USABLE), NONE),
] + [((NO_KERNEL, n_i, lane, cap), NONE)      # a batch without k_sel_stretch: no lane writes, nothing wraps
     for n_i in (1, 8) for lane in range(8) for cap in (1, 9, USABLE)]


def test_slot_decision_on_hand_derived_cases(program):
    got = program(["slot %d %d %d %d" % args for args, _ in SLOT_TABLE])
    assert len(got) == len(SLOT_TABLE)
    for (args, want), line in zip(SLOT_TABLE, got):
        assert int(line) == want, args


def _arrivals(rng, n_slices, kind):
    n_i = {"mixed": lambda: rng.randint(1, SEL_REQ), "full": lambda: SEL_REQ, "single": lambda: 1,
           "mostly_full": lambda: SEL_REQ if rng.random() < 0.9 else rng.randint(1, SEL_REQ)}[kind]
    arr = [(s, n_i()) for s in range(n_slices) if kind == "full" or rng.random() < 0.8]  # (slices without a stretch reserve nothing)
    rng.shuffle(arr)
    return arr


def _caps(total):
    return sorted({1, 7, 8, 9, 64, 61, 16, 13, max(1, total - 1), total, total + 1, max(1, total // 2), max(1, total // 3)})


def _model(arr, cap):
    """what must happen, stated apart from the header: a slice's requests are taken iff its reservation ends at or in front of the
    capacity, else all of them go to k_gap_fix; is some reservation cut by the capacity?"""
    base, taken, straddle = 0, set(), False
    for s, n_i in arr:
        if base + n_i <= cap:
            taken.add(s)
        elif base < cap:
            straddle = True
        base += n_i
    return taken, straddle, min(base, cap)


def _sim(program, rule, cap, poison, n_slices, arr):
    line = "sim %d %d %d %d %d " % (rule, cap, poison, n_slices, len(arr)) + " ".join("%d %d" % a for a in arr)
    f = program([line])[0].split()
    first_stale, other_stale, beyond, out_of_array, n_req = map(int, f[:5])
    per_slice = [tuple(map(int, x.split(":"))) for x in f[5:]]
    return first_stale, other_stale, beyond, out_of_array, n_req, per_slice


@pytest.mark.parametrize("kind", ["mixed", "full", "single", "mostly_full"])
@pytest.mark.parametrize("poison", [0, 1])
def test_walk_meets_only_what_this_round_wrote(program, kind, poison):
    rng = random.Random(1000 + poison)
    straddles = 0
    for trial in range(12):
        n_slices = rng.choice([1, 2, 5, 40, 200])
        arr = _arrivals(rng, n_slices, kind)
        total = sum(n for _, n in arr)
        n_i_of = dict(arr)
        for cap in _caps(total):
            taken, straddle, n_req = _model(arr, cap)
            straddles += straddle
            first_stale, other_stale, beyond, out_of_array, got_req, per_slice = _sim(program, 0, cap, poison, n_slices, arr)
            ctx = (kind, poison, trial, cap, total)
            assert got_req == n_req, ctx
            assert first_stale == 0, ctx       # every entry the walk takes as a slice's first request is this round's
            assert other_stale == 0, ctx       # every other entry it visits is a tombstone or a later request of this round
            assert beyond == 0 and out_of_array == 0, ctx   # nothing is written or used at or behind the capacity
            for s, (written, pushed, took) in enumerate(per_slice):
                n_i = n_i_of.get(s, 0)
                if s in taken:                 # all of the slice's stretches in the array, taken by exactly one wave
                    assert (written, pushed, took) == (n_i, 0, 1), (ctx, s)
                else:                          # all of them to k_gap_fix, none taken: a slice's stretches stay together
                    assert (written, pushed, took) == (0, n_i, 0), (ctx, s)
    assert kind == "single" or straddles > 10  # (reservations of one entry cannot be cut)


def test_the_rule_before_this_one_fails_where_a_reservation_is_cut(program):
    """base + n_i <= capacity or nothing: entries between the base of a cut reservation and the capacity keep what the array held,
    and the walk visits them.  Where no reservation is cut, the two rules do the same."""
    rng = random.Random(7)
    caught = fine = 0
    for trial in range(12):
        n_slices = rng.choice([5, 40, 200])
        arr = _arrivals(rng, n_slices, "mostly_full")
        total = sum(n for _, n in arr)
        for cap in _caps(total):
            _, straddle, _ = _model(arr, cap)
            for poison in (0, 1):
                old = _sim(program, 1, cap, poison, n_slices, arr)
                new = _sim(program, 0, cap, poison, n_slices, arr)
                if straddle:
                    assert old[0] + old[1] > 0, (trial, cap, poison)   # stale entries met: the bug
                    caught += 1
                else:
                    assert old == new, (trial, cap, poison)
                    fine += 1
                assert new[0] == new[1] == 0
    assert caught > 20 and fine > 20
