"""The teeth of the tests of launch_max_scan_u64 and of its two users, shown on the CPU with tests/_maxscan_model.py: every input of
tests/test_gpu_primitives.py::test_maxscan64, every table of tests/test_gpu_lift.py::test_lookups_that_live_on_the_carries and both
cases of tests/test_gpu_assess.py::test_chains_under_a_long_chain_behind_a_carry would come out WRONG -- through the very lookup the
device does -- if the scan had the carry fault the input is there for.  The lookups over the running maximum are bisections
(lift.h) and a sum that a wrong maximum often leaves alone (assess.h), so this is not a matter of course: with the long piece at
place 500, 1 500 or 100 000 of a 262 445-piece record a dropped round carry leaves 301 words of rmax wrong and the candidates of every
feature behind them as they were, because the first probes fall into the part that is still right."""
import numpy as np
import pytest

from tests import _cover_scale as CS, _lift_cases as LC, _maxscan_model as M

# (long_at, n_short) -> the faults the table is there for.  No table shows tiles_inclusive: a maximum that arrives early only widens
# a feature's candidates, and lift_count skips the ones that end in front of it; the primitive's and the assessment's tests show it
LIFT_TEETH = {(1023, 4400): ("tile_carry",), (1024, 4400): ("tile_carry",), (262143, 262444): ("tile_carry", "round_carry"),
              (262144, 262444): ("tile_carry",)}
# (m0, m1) -> the faults
COVER_CASES = CS.CARRY_CASES
COVER_TEETH = {(1022, 1500): ("tile_carry", "tiles_inclusive"), (262142, 1500): ("tile_carry", "round_carry", "tiles_inclusive")}


def test_the_model_without_a_fault_is_the_running_maximum():
    inputs = [M.pattern_input(n, pattern, at) for n, pattern, at in M.cases() if n <= 4097 or (n == 262145 and pattern != "single")]
    inputs += [M.pattern_input(262145, "single", at) for at in M.single_places(262145)]
    inputs += [LC.index_words(LC.carry_case(long_at, 4400)[0])[1] for long_at in (1023, 1024)] + [CS.sorted_chains(1022, 1500)[1]]
    assert len(inputs) > 60
    for a in inputs:
        want = np.maximum.accumulate(a)
        assert (M.max_scan(a) == want).all()
        front = M.max_scan(a, exclusive=True)
        assert front[0] == 0 and (front[1:] == want[:-1]).all()


def test_the_teeth_name_every_carry_fault():
    users = list(LIFT_TEETH.values()) + list(COVER_TEETH.values())
    assert {f for _, faults in M.TEETH.values() for f in faults} | {f for v in users for f in v} == set(M.FAULTS)
    assert set(LIFT_TEETH) == set(LC.CARRY_CASES) and set(COVER_TEETH) == set(COVER_CASES)
    assert {(p, at) for _, p, at in M.cases()} == set(M.TEETH) and all(faults for _, faults in M.TEETH.values())
    assert M.TEETH[("top_bit", None)][1][0] == "signed"
    for fault in ("tile_carry", "round_carry", "tiles_inclusive"):   # each carry: in the primitive's own test, and in a user's
        assert any(fault in faults for _, faults in M.TEETH.values())
        assert any(fault in v for v in users)


@pytest.mark.parametrize("pattern,at", sorted(M.TEETH, key=str), ids=str)
def test_teeth_of_the_patterns(pattern, at):
    n, faults = M.TEETH[(pattern, at)]
    assert (n, pattern, at) in M.cases()   # a case the GPU test runs
    a = M.pattern_input(n, pattern, at)
    want = np.maximum.accumulate(a)
    for fault in faults:
        assert (M.max_scan(a, fault) != want).any(), fault


@pytest.mark.parametrize("long_at,n_short", LC.CARRY_CASES)
def test_teeth_of_the_lift_tables(long_at, n_short):
    table, source_length, features, statuses = LC.carry_case(long_at, n_short)
    status, part_first, _parts = LC.carry_expected(long_at, n_short)
    assert status == statuses
    key, word, start, end = LC.index_words(table)
    record = (key >> np.uint64(32)).astype(np.int64)
    assert len(key) == n_short + 1 + LC.CARRY_SECOND + 1 and int(key[long_at]) == 3 * long_at - 1 and int(word[long_at]) == source_length[0]
    rmax = np.maximum.accumulate(word)
    # the places of the index that give the restatement its parts, and the header's own lookup over the right array: it holds them all
    places, right = [], []
    for i, (r, a, b) in enumerate(features):
        places.append(np.flatnonzero((record == r) & (start < b) & (end > a)))
        assert len(places[i]) == part_first[i + 1] - part_first[i]
        lo, hi = M.lift_range(key, rmax, r, a, b)
        assert ((places[i] >= lo) & (places[i] < hi)).all()
        right.append((lo, hi))
    assert right[0] == (long_at, n_short + 1) and right[4] == (long_at - 10, long_at - 9)   # (the far end walks all of them, the front one piece)
    for fault in LIFT_TEETH[(long_at, n_short)]:
        wrong = M.max_scan(word, fault)
        assert (wrong != rmax).any(), fault
        lost = []
        for i, (r, a, b) in enumerate(features):
            lo, hi = M.lift_range(key, wrong, r, a, b)
            if (lo, hi) != right[i] and ((places[i] < lo) | (places[i] >= hi)).any():
                lost.append(i)
        assert lost, fault   # a feature whose candidates differ AND leave out a piece the restatement lifts it through
        if fault == "round_carry":
            assert set(lost) >= {0, 1, 2, 3}   # everything behind the long piece on record 0


@pytest.mark.parametrize("m0,m1", COVER_CASES)
def test_teeth_of_the_cover_cases(m0, m1):
    key, word = CS.sorted_chains(m0, m1)
    want = sum(CS.chain_end(m) - 1000 for m in (m0, m1))
    assert len(key) == m0 + m1 + 2 and int(key[m0 + 1]) == 1 << 32 | 1000 and (m0 + 1) % 1024 == 1023
    assert CS.covered(key, word, M.max_scan(word, exclusive=True)) == want
    for fault in COVER_TEETH[(m0, m1)]:
        assert CS.covered(key, word, M.max_scan(word, fault, exclusive=True)) != want, fault
