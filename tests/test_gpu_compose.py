"""GPU tests of mxg_compose_pieces (csrc/compose.hip; include/ntjoin_mx.h, row f11) against the restatement of its contract
(tests/_compose_restatement.py): the hand-made cases and the seeded fuzz of the CPU test, outer piece counts at the scan's tile and
level borders, inner records of 1 and of 1000 pieces, three rounds composed either way, and the refusals."""
import numpy as np
import pytest

from ntjoin_amd import capi
from ntjoin_amd.engine import MxEngine, MxError
from tests import _compose_cases as cases, _compose_restatement as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    with MxEngine(k=32, w=100) as engine:
        yield engine


def compose(eng, outer, inner):
    orows, ofirst = cases.flatten(outer)
    irows, ifirst = cases.flatten(inner)
    pieces, first = eng.compose_pieces(orows, ofirst, irows, ifirst)
    assert pieces.dtype == MxEngine.SEQ_PIECE and first.dtype == np.uint64
    assert len(first) == len(outer) + 1 and int(first[0]) == 0 and int(first[-1]) == len(pieces)
    return cases.unflatten(pieces.tolist(), first)


@pytest.mark.parametrize("name", sorted(cases.HAND))
def test_hand_made_cases(eng, name):
    outer = cases.HAND[name]
    got = compose(eng, outer, cases.INNER)
    assert got == R.compose(outer, cases.INNER)
    cases.check_spelling(cases.BASE_LEN, cases.INNER, outer, got)


def test_seeded_fuzz(eng):
    for seed in range(120):
        base_len, inner, outer = cases.fuzz_case(seed, inner_pieces=(None, 1, 37)[seed % 3], outer_pieces=(4, 1, 12)[seed % 3])
        got = compose(eng, outer, inner)
        assert got == R.compose(outer, inner), seed
        cases.check_spelling(base_len, inner, outer, got, seed)


@pytest.mark.parametrize("n_pieces", [1, 255, 256, 257, 1023, 1024, 1025, 65537])
def test_outer_piece_counts_at_the_scan_borders(eng, n_pieces):
    "256 pieces per block of the kernels, 1024 per tile of the scan, 4096 tiles' sums... and one past 2^16; records of one piece"
    base_len, inner, outer = cases.fuzz_case(n_pieces, n_outer=n_pieces, outer_pieces=1)
    assert sum(len(rec) for rec in outer) == n_pieces
    got = compose(eng, outer, inner)
    assert got == R.compose(outer, inner)
    cases.check_spelling(base_len, inner, outer, got)


@pytest.mark.parametrize("n_pieces", [257, 4097])
def test_one_outer_record_of_many_pieces(eng, n_pieces):
    "the join of gaps and the records' starts when one record spans blocks and tiles"
    rng = cases.random.Random(n_pieces)
    base_len, inner, _ = cases.fuzz_case(n_pieces)
    outer = cases.random_table(rng, 2, [R.record_length(rec) for rec in inner], max_pieces=1)
    big = []
    while len(big) < n_pieces:
        big.extend(cases.random_table(rng, 1, [R.record_length(rec) for rec in inner], max_pieces=6, gap_p=0.5)[0])
    outer.insert(1, big[:n_pieces])
    got = compose(eng, outer, inner)
    assert got == R.compose(outer, inner)
    cases.check_spelling(base_len, inner, outer, got)


@pytest.mark.parametrize("inner_pieces", [1, 1000])
def test_inner_records_of_1_and_1000_pieces(eng, inner_pieces):
    for seed in (1, 2, 3):
        base_len, inner, outer = cases.fuzz_case(seed, n_outer=60, inner_pieces=inner_pieces, outer_pieces=5)
        assert all(len(rec) == inner_pieces for rec in inner)
        got = compose(eng, outer, inner)
        assert got == R.compose(outer, inner), seed
        cases.check_spelling(base_len, inner, outer, got, seed)
        if inner_pieces == 1000:
            assert max(len(rec) for rec in got) > 500   # (some outer piece did span most of a record)


def test_three_rounds_compose_either_way(eng):
    for seed in range(10):
        base_len, t1, t2 = cases.fuzz_case(seed)
        t3 = cases.random_table(cases.random.Random(1000 + seed), 3, [R.record_length(rec) for rec in t2])
        assert compose(eng, t3, compose(eng, t2, t1)) == compose(eng, compose(eng, t3, t2), t1) == R.compose(t3, R.compose(t2, t1))


def test_no_outer_records(eng):
    assert compose(eng, [], cases.INNER) == []
    assert compose(eng, [], []) == []


@pytest.mark.parametrize("name", sorted(cases.REFUSED))
def test_refusals(eng, name):
    inner, outer, code = cases.REFUSED[name]
    with pytest.raises(MxError) as err:
        compose(eng, outer, inner)
    assert err.value.code == {R.EINVAL: capi.MXG_EINVAL, R.ELIMIT: capi.MXG_ELIMIT}[code]
    assert "mxg_compose_pieces" in str(err.value)
    # the handle is as it was: the next call answers
    assert compose(eng, cases.HAND["record_of_one_piece"], cases.INNER) == R.compose(cases.HAND["record_of_one_piece"], cases.INNER)


def test_result_of_2_31_pieces_is_refused_before_it_is_made(eng):
    "65 537 outer pieces over an inner record of 32 768 pieces: 2^31 + 32 768 pieces, known from the count alone"
    inner = [[(0, j, j + 1, R.FWD) for j in range(32768)]]
    outer = [[(0, 0, 32768, R.REV)] * 65537]
    with pytest.raises(MxError) as err:
        compose(eng, outer, inner)
    assert err.value.code == capi.MXG_ELIMIT and "2^31" in str(err.value)
    assert compose(eng, [[(0, 5, 9, R.REV)]], inner) == [[(0, j, j + 1, R.REV) for j in (8, 7, 6, 5)]]
