"""GPU tests of mxg_lift_prepare / mxg_lift_intervals / mxg_lift_bed (include/ntjoin_mx.h, row f15) against the restatement of the
contract (tests/_lift_restatement.py: a linear scan over all pieces, no index) on the cases of tests/_lift_cases.py, and past the
borders of the kernels: 256 threads a block, 1024 elements a tile of the scans and of the sort, 256 tiles a round of the running
maximum's second pass (262 144 pieces), one more 8-bit digit of the sort per 256-fold of source records.  The shapes are the smallest
that cross them; the largest table has 263 446 pieces, far below the 4096 tiles at which the 32-bit scans take a second pass."""
import numpy as np
import pytest

from ntjoin_amd import capi
from ntjoin_amd.engine import MxEngine, MxError
from tests import _lift_cases as cases, _lift_restatement as R

pytestmark = pytest.mark.gpu

BORDERS = [1, 255, 256, 257, 1023, 1024, 1025, 65537]


@pytest.fixture(scope="module")
def eng():
    with MxEngine(k=32, w=100) as engine:
        yield engine


def prepare(eng, table, source_length):
    rows, first = cases.CC.flatten(table)
    eng.lift_prepare(np.asarray(rows, dtype=np.uint32).reshape(-1, 4), first, source_length)


def lift(eng, features, whole_only=False):
    f = np.asarray(features, dtype=np.uint32).reshape(-1, 3)
    status, part_first, parts = eng.lift_intervals(f[:, 0], f[:, 1], f[:, 2], whole_only=whole_only)
    return status.tolist(), part_first.tolist(), [tuple(int(x) for x in p) for p in parts.tolist()]


def check(eng, table, source_length, features, whole_only=False, seed=0, spelling=True):
    prepare(eng, table, source_length)
    got = lift(eng, features, whole_only)
    assert got == R.lift(table, source_length, features, whole_only)
    if spelling:
        cases.check_spelling(table, source_length, features, *got, seed=seed, whole_only=whole_only)
    return got


def test_hand_made_cases(eng):
    names = sorted(cases.HAND)
    got = check(eng, cases.TABLE, cases.SOURCE_LEN, [cases.HAND[n][0] for n in names])
    for i, n in enumerate(names):
        assert (got[0][i], got[2][got[1][i]:got[1][i + 1]]) == cases.HAND[n][1:], n


def test_whole_only(eng):
    names = sorted(cases.HAND)
    features = [cases.HAND[n][0] for n in names]
    status, part_first, parts = check(eng, cases.TABLE, cases.SOURCE_LEN, features, whole_only=True)
    assert status == [cases.HAND[n][1] for n in names]   # (a feature that is not WHOLE keeps its status)
    assert parts == [p for n in names if cases.HAND[n][1] == R.WHOLE for p in cases.HAND[n][2]]
    assert all((part_first[i + 1] - part_first[i]) == (1 if s == R.WHOLE else 0) for i, s in enumerate(status))


def test_seeded_fuzz(eng):
    for seed in range(210):
        table, source_length, features = cases.fuzz_case(seed)
        check(eng, table, source_length, features, whole_only=seed % 7 == 0, seed=seed)


@pytest.mark.parametrize("n_pieces", BORDERS)
def test_sequence_piece_counts_at_the_borders(eng, n_pieces):
    "three source records, so that a feature's candidates run over blocks and tiles of the index; few features: the restatement is linear"
    table, source_length = cases.sized_case(n_pieces, 3)
    assert sum(p[3] != R.GAP for rec in table for p in rec) == n_pieces
    check(eng, table, source_length, cases.sized_features(24 if n_pieces < 65537 else 12, 3, seed=n_pieces), seed=n_pieces)


@pytest.mark.parametrize("n_features", BORDERS)
def test_feature_counts_at_the_borders(eng, n_features):
    table, source_length = cases.sized_case(9, 4, seed=1)
    features = cases.sized_features(n_features, 4, seed=n_features)
    status, part_first, parts = check(eng, table, source_length, features, spelling=n_features <= 1025)
    assert len(status) == n_features and len(set(status)) >= min(n_features, 3)


@pytest.mark.parametrize("n_source", [1, 2, 256, 257, 65537])
def test_source_record_counts_across_the_sort_s_digits(eng, n_source):
    "the key is 32 bits of start and 0, 1, 8, 9 and 17 bits of record: four to seven passes of the sort"
    table, source_length = cases.sized_case(700, n_source, seed=2)
    rng = cases.random.Random(n_source)
    named = [p for rec in table for p in rec if p[3] != R.GAP]
    features = cases.sized_features(60, n_source, seed=3)
    for _ in range(140):   # (on records that pieces name: a random record of 65 537 is named by none)
        r, a, b, _ = rng.choice(named)
        lo = rng.randrange(0, b)
        features.append((r, lo, rng.randint(max(lo, a) + 1, 64)))
    status = check(eng, table, source_length, features, seed=n_source)[0]
    assert status.count(R.LOST) < len(status) // 2


def test_one_source_record_in_4097_pieces_under_a_feature_that_spans_them(eng):
    rng = cases.random.Random(4097)
    pieces = [(0, 3 * j, 3 * j + 2, rng.choice((R.FWD, R.REV))) for j in range(4097)]   # (every third base is in no piece)
    rng.shuffle(pieces)
    table, at = [], 0
    while at < len(pieces):
        n = rng.randint(1, 40)
        table.append(pieces[at:at + n])
        at += n
    L = 3 * 4097
    features = [(0, 0, L), (0, 1, L - 2), (0, 2, 3), (0, 3000, 3002), (0, 2999, 9001)]
    status, part_first, parts = check(eng, table, [L], features)
    assert status == [R.PARTIAL, R.PARTIAL, R.LOST, R.WHOLE, R.PARTIAL]
    assert part_first[1] == 4097 and [p[3] for p in parts[:4097]] == [3 * j for j in range(4097)]


@pytest.mark.parametrize("long_at,n_short", cases.CARRY_CASES)
def test_lookups_that_live_on_the_carries(eng, long_at, n_short):
    """one long piece on the last place of tile 0 and the first of tile 1, on the last place of the first round of k_pt_max_tiles
    (256 tiles) and the first of the second, over everything behind it; a second record with a long piece on the last place of a later
    tile.  tests/test_maxscan_model_cpu.py shows that these features lose their parts when rmax lacks the carry in question"""
    table, source_length, features, statuses = cases.carry_case(long_at, n_short)
    prepare(eng, table, source_length)
    got = lift(eng, features)
    assert got == cases.carry_expected(long_at, n_short) and got[0] == statuses
    if n_short < 10000:
        cases.check_spelling(table, source_length, features, *got)


def test_nothing_to_lift_through_and_nothing_to_lift(eng):
    features = [(0, 0, 5), (1, 3, 9), (7, 0, 1), (0, 4, 4)]
    for table in ([], [[(0, 0, 5, R.GAP)], [(0, 0, 1, R.GAP), (0, 0, 2, R.GAP)]]):   # n_records == 0; no sequence piece
        got = check(eng, table, cases.SOURCE_LEN, features)
        assert got == ([R.LOST, R.LOST, R.INVALID, R.INVALID], [0] * 5, [])
    assert check(eng, cases.TABLE, cases.SOURCE_LEN, []) == ([], [0], [])   # n == 0
    prepare(eng, [], [])   # no source records either
    assert lift(eng, [(0, 0, 1)]) == ([R.INVALID], [0, 0], [])


# ---- mxg_lift_bed --------------------------------------------------------------------------------------------------------------------
def bed_files(tmp_path, table, source_length, source_names, scaffold_names, data, whole_only=False, unlifted=True):
    "a fresh engine: a handle reads a knob once"
    bed = tmp_path / "in.bed"
    bed.write_bytes(data)
    with MxEngine(k=32, w=100) as e:
        prepare(e, table, source_length)
        st = e.lift_bed(bed, [n.decode() for n in source_names], [n.decode() for n in scaffold_names], tmp_path / "lifted.bed",
                        tmp_path / "unlifted.bed" if unlifted else None, whole_only=whole_only)
        st["knobs"] = e.knobs().split()
    return (tmp_path / "lifted.bed").read_bytes(), (tmp_path / "unlifted.bed").read_bytes() if unlifted else None, st


HAND_BED = (cases.TABLE, cases.SOURCE_LEN, cases.SOURCE_NAMES, cases.SCAFFOLD_NAMES, cases.BED)


@pytest.mark.parametrize("whole_only", [False, True])
def test_bed_file_is_the_restatement_s(tmp_path, whole_only):
    want = R.lift_bed(*HAND_BED, whole_only)
    assert b"ntJoin0\t350\t400\tsplit\t0\t+\nntJoin1\t0\t100\tsplit\t0\t+\n" in want[0] or whole_only   # (a SPLIT feature: two lines)
    lifted, unlifted, st = bed_files(tmp_path, *HAND_BED, whole_only=whole_only)
    assert not [k for k in st.pop("knobs") if k.startswith("MXG_LIFT_")]   # the defaults
    assert (lifted, unlifted, st) == want


@pytest.mark.parametrize("win", [1, 7, 4096])
def test_bed_files_do_not_depend_on_the_window(tmp_path, monkeypatch, win):
    "1: a border between all bytes; 7: inside numbers, names and between the two lines of the SPLIT feature; 4096: one window"
    monkeypatch.setenv("MXG_LIFT_WIN", str(win))
    lifted, unlifted, st = bed_files(tmp_path, *HAND_BED)
    assert f"MXG_LIFT_WIN={win}" in st.pop("knobs") and len(lifted) > 400   # (hundreds of windows of 1 byte, dozens of 7)
    assert (lifted, unlifted, st) == R.lift_bed(*HAND_BED)


@pytest.mark.parametrize("batch", [1, 40, 200])
def test_bed_files_do_not_depend_on_the_batch(tmp_path, monkeypatch, batch):
    "1: every line is a batch of its own; 40 and 200: the border falls inside a would-be line and moves back to its start"
    monkeypatch.setenv("MXG_LIFT_BATCH", str(batch))
    monkeypatch.setenv("MXG_LIFT_WIN", "13")
    assert max(len(ln) for ln in cases.BED.split(b"\n")) > 40
    lifted, unlifted, st = bed_files(tmp_path, *HAND_BED)
    assert f"MXG_LIFT_BATCH={batch}" in st.pop("knobs")
    assert (lifted, unlifted, st) == R.lift_bed(*HAND_BED)


def test_bed_fuzz_and_no_unlifted_file(tmp_path):
    table, source_length, features = cases.fuzz_case(5, n_features=300)
    src = [b"s%d" % r for r in range(len(source_length))]
    dst = [b"ntJoin%d" % r for r in range(len(table))]
    data = b"".join(src[r] + b"\t%d\t%d\tf%d\t0\t%s\n" % (a, b, i, b"+-."[i % 3:i % 3 + 1]) if r < len(src) else b"nowhere\t%d\t%d\n" % (a, b)
                    for i, (r, a, b) in enumerate(features))
    want = R.lift_bed(table, source_length, src, dst, data)
    lifted, unlifted, st = bed_files(tmp_path, table, source_length, src, dst, data, unlifted=False)
    st.pop("knobs")
    assert (lifted, unlifted) == (want[0], None) and st == dict(want[2], unlifted_bytes=0)
    for empty in (b"", b"\n", b"#only a comment"):
        assert bed_files(tmp_path, table, source_length, src, dst, empty)[:2] == (b"", b"")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_no_prepared_index(tmp_path):
    with MxEngine(k=32, w=100) as e:
        with pytest.raises(MxError) as err:
            e.lift_intervals([0], [0], [1])
        assert err.value.code == capi.MXG_EINVAL and "mxg_lift_prepare" in str(err.value)
        (tmp_path / "x.bed").write_bytes(b"a\t0\t1\n")
        with pytest.raises(MxError) as err:
            e.lift_bed(tmp_path / "x.bed", [], [], tmp_path / "l.bed")
        assert err.value.code == capi.MXG_EINVAL and not (tmp_path / "l.bed").exists()
        prepare(e, cases.TABLE, cases.SOURCE_LEN)   # the next call answers
        assert lift(e, [(0, 10, 50)]) == ([R.WHOLE], [0, 1], [(0, 10, 50, 10, 0)])


@pytest.mark.parametrize("name", sorted(cases.REFUSED))
def test_refused_tables(eng, name):
    table, source_length, code = cases.REFUSED[name]
    prepare(eng, cases.TABLE, cases.SOURCE_LEN)
    with pytest.raises(MxError) as err:
        prepare(eng, table, source_length)
    assert err.value.code == {R.EINVAL: capi.MXG_EINVAL, R.ELIMIT: capi.MXG_ELIMIT}[code] and "mxg_lift_prepare: table" in str(err.value)
    if name == "piece_beyond_its_source_record":
        assert "table record 1 piece 0 {1, 0, 501, 1} is not inside its inner record" in str(err.value)
    if name == "piece_names_no_source_record":
        assert "table record 0 piece 1 {6, 0, 1, 0} names a record that does not exist" in str(err.value)
    with pytest.raises(MxError) as err:   # a failed prepare leaves no index, not the one before
        lift(eng, [(0, 10, 50)])
    assert err.value.code == capi.MXG_EINVAL
    prepare(eng, cases.TABLE, cases.SOURCE_LEN)   # the next call answers
    assert lift(eng, [(0, 10, 50)]) == ([R.WHOLE], [0, 1], [(0, 10, 50, 10, 0)])


def test_2_31_parts_are_refused_from_the_count_alone(eng, tmp_path):
    "65 537 features over a record of 32 768 one-base pieces: 2^31 + 32 768 parts, known before anything is scanned or emitted"
    prepare(eng, [[(0, j, j + 1, R.FWD) for j in range(32768)]], [32768])
    with pytest.raises(MxError) as err:
        eng.lift_intervals(np.zeros(65537, np.uint32), np.zeros(65537, np.uint32), np.full(65537, 32768, np.uint32))
    assert err.value.code == capi.MXG_ELIMIT and "2^31" in str(err.value) and str(2 ** 31 + 32768) in str(err.value)
    # the index stands: the next call answers, and so does the same call under whole_only, which has no parts to refuse
    assert lift(eng, [(0, 5, 9)]) == ([R.SPLIT], [0, 4], [(0, j, j + 1, j, 0) for j in (5, 6, 7, 8)])
    status, part_first, parts = eng.lift_intervals(np.zeros(65537, np.uint32), np.zeros(65537, np.uint32), np.full(65537, 32768, np.uint32), whole_only=True)
    assert set(status.tolist()) == {R.SPLIT} and len(parts) == 0 and int(part_first[-1]) == 0
