"""GPU tests of the device TSV writer (write_tsv_device in ntjoin_amd/csrc/ingest.hip: k_tsv_len, k_tsv_tile_sum, k_tsv_scan_tiles,
k_tsv_offsets, k_tsv_entries, k_tsv_ids) on input the sketch kernels never give it: hashes and positions of every decimal length,
record tables of every shape, minimizer counts on both sides of the scan's tiles (1024) and passes (4 194 304), a window border
through every byte of the text (MXG_TSV_WIN), and k on both sides of the switch to the host writer (200).

The sketch is handed over with MxEngine.add_minimizers; write_tsv(..., with_seq=False) of such an assembly is formatted on the device
(host_io.cpp write_tsv: a sketch, no host text, not sharded, k <= 200, MXG_HOST_TSV unset, no k-mer column asked for).  Which writer ran
is witnessed by the line "[mxg] write_tsv_device ..." that MXG_DEBUG_IO=1 prints when, and only when, the device writer ran.

Reference: plain Python, `id + "\\t" + " ".join(entries) + "\\n"` per record.  Every comparison is byte for byte.
Per file: (a) device file = reference; (b) the host writer (MXG_HOST_TSV=1) writes the same bytes -- on a second handle given the
same arrays, since a handle parses a knob once, at its first use, and the first write_tsv has then seen MXG_HOST_TSV unset;
(c) add_tsv of the device file gives the input back.  (c) needs entries of exactly three ':'-fields, as read_minimizers of the
reference does: that is the file with positions AND strands (the parser ignores the third field); a file of
`hash:pos` entries is refused by the parser, which test_digits asserts.  The parser skips records without minimizers, as
read_minimizers does, so (c) compares with the input's records that have some.

Strand: add_minimizers installs every minimizer as forward; set_sketch_device on that assembly replaces the sketch by device arrays
that carry a strand of their own, so the strand column does vary here, and what is expected is get_sketch()["forward"] of the
handle that wrote the file."""
import random
import re

import numpy as np
import pytest

from ntjoin_amd.engine import MxEngine, MxError

pytestmark = pytest.mark.gpu

DEVICE_LINE = "[mxg] write_tsv_device"
TILE = 1024                 # entries per tile of the offset scan
PASS = 256 * 16 * TILE      # entries per pass of k_tsv_scan_tiles: 4 194 304
WIN = 64 << 20              # bytes per output window


@pytest.fixture(autouse=True)
def tsv_env(monkeypatch):
    for name in ("MXG_HOST_TSV", "MXG_HOST_INGEST", "MXG_TSV_WIN"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("MXG_DEBUG_IO", "1")
    return monkeypatch


# ---------------------------------------------------------------------------------------------------------------
# reference and helpers
# ---------------------------------------------------------------------------------------------------------------
def reference_text(hashes, pos, record, ids, with_pos, with_strand, forward=None):
    first = np.searchsorted(record, np.arange(len(ids) + 1))
    lines = []
    for r, rid in enumerate(ids):
        lo, hi = int(first[r]), int(first[r + 1])
        cols = [map(str, hashes[lo:hi].tolist())]
        if with_pos:
            cols.append(map(str, pos[lo:hi].tolist()))
        if with_strand:
            cols.append("+" if f else "-" for f in forward[lo:hi].tolist())
        lines.append(rid + "\t" + " ".join(map(":".join, zip(*cols))) + "\n")
    return "".join(lines).encode("ascii")


def same_bytes(got, want, what):
    if got == want:
        return
    n = min(len(got), len(want))
    a, b = np.frombuffer(got, dtype=np.uint8, count=n), np.frombuffer(want, dtype=np.uint8, count=n)
    diff = np.flatnonzero(a != b)
    at = int(diff[0]) if len(diff) else n
    pytest.fail(f"{what}: {len(got)} bytes against {len(want)}, first difference at byte {at}: "
                f"{got[max(0, at - 30):at + 30]!r} against {want[max(0, at - 30):at + 30]!r}")


def install(eng, hashes, pos, record, ids, forward=None):
    a = eng.add_minimizers("t", 1.0, hashes, pos, record, ids)
    if forward is not None and len(hashes):
        import torch
        dev = [torch.from_numpy(x).cuda() for x in (hashes.view(np.int64), pos.view(np.int32), record.view(np.int32), forward)]
        eng.set_sketch_device(a, *(t.data_ptr() for t in dev), len(hashes))
        del dev   # (the handle copied them)
    return a


def write(capfd, path, sketch, with_pos, with_strand, device=True):
    """one fresh handle -> (the file's bytes, its get_sketch, its knobs); with a capfd, asserts which writer ran"""
    hashes, pos, record, ids, forward = sketch
    if capfd is not None:
        capfd.readouterr()
    with MxEngine(k=32, w=100) as eng:
        a = install(eng, hashes, pos, record, ids, forward if with_strand else None)
        eng.write_tsv(a, str(path), with_pos=with_pos, with_strand=with_strand, with_seq=False)
        sk = eng.get_sketch(a)
        knobs = eng.knobs().split()
    if capfd is not None:
        assert (DEVICE_LINE in capfd.readouterr().err) == device
    with open(path, "rb") as fh:
        return fh.read(), sk, knobs


def check_file(capfd, env, tmp_path, sketch, with_pos, with_strand, host=True, roundtrip=True):
    """checks (a), (b), (c) of the module's docstring -> the device file's bytes"""
    hashes, pos, record, ids, forward = sketch
    got, sk, knobs = write(capfd, tmp_path / "dev.tsv", sketch, with_pos, with_strand)
    assert not [k for k in knobs if k.startswith(("MXG_HOST_TSV", "MXG_TSV_WIN"))]
    for key, arr in (("out_hash", hashes), ("pos", pos), ("record", record)):
        assert np.array_equal(sk[key], arr), key
    if with_strand and len(hashes):
        assert np.array_equal(sk["forward"], forward)
    want = reference_text(hashes, pos, record, ids, with_pos, with_strand, sk["forward"])
    same_bytes(got, want, "device writer against the reference")
    if host:
        env.setenv("MXG_HOST_TSV", "1")
        by_host, _, knobs = write(capfd, tmp_path / "host.tsv", sketch, with_pos, with_strand, device=False)
        env.delenv("MXG_HOST_TSV")
        assert "MXG_HOST_TSV=1" in knobs
        same_bytes(by_host, want, "host writer against the reference")
    if roundtrip and with_pos and with_strand:
        with MxEngine(k=32, w=100) as eng:
            a = eng.add_tsv("back", 1.0, str(tmp_path / "dev.tsv"))
            back = eng.get_sketch(a)
        first = np.searchsorted(record, np.arange(len(ids) + 1))
        kept = np.flatnonzero(first[1:] > first[:-1])          # the parser skips records without minimizers
        renumber = np.zeros(len(ids) + 1, dtype=np.uint32)
        renumber[kept] = np.arange(len(kept), dtype=np.uint32)
        assert np.array_equal(back["out_hash"], hashes) and np.array_equal(back["pos"], pos)
        assert np.array_equal(back["record"], renumber[record])
        assert back["record_ids"] == [ids[r] for r in kept.tolist()]
    return got


def random_digits(rng, n, max_digits, top):
    """n values whose decimal length is uniform over 1 .. max_digits (the longest length reaches up to `top`)"""
    d = rng.integers(1, max_digits + 1, size=n)
    lo = np.array([0] + [10 ** e for e in range(1, max_digits)], dtype=np.uint64)[d - 1]
    hi = np.array([min(10 ** e - 1, top) for e in range(1, max_digits + 1)], dtype=np.uint64)[d - 1]
    return rng.integers(lo, hi, dtype=np.uint64, endpoint=True)


def random_sketch(seed, n, ids, counts=None):
    """n minimizers with hashes of 1 to 20 and positions of 1 to 10 digits over the records `ids`; counts: minimizers per record
    (default: cut at random places, with records without minimizers among them)"""
    rng = np.random.default_rng(seed)
    if counts is None:
        cuts = np.sort(rng.integers(0, n + 1, size=len(ids) - 1))
        cuts[1::5] = cuts[0::5][:len(cuts[1::5])]              # every fifth record is empty for certain
        counts = np.diff(np.concatenate(([0], np.sort(cuts), [n])))
    counts = np.asarray(counts, dtype=np.int64)
    assert counts.sum() == n and len(counts) == len(ids)
    hashes = random_digits(rng, n, 20, 2 ** 64 - 1)
    pos = random_digits(rng, n, 10, 2 ** 32 - 1).astype(np.uint32)
    record = np.repeat(np.arange(len(ids), dtype=np.uint32), counts)
    forward = (rng.random(n) < 0.6).astype(np.uint8)
    return hashes, pos, record, list(ids), forward


# ---------------------------------------------------------------------------------------------------------------
# 1. digits
# ---------------------------------------------------------------------------------------------------------------
DIGIT_HASHES = ([0] + [10 ** d + e for d in range(1, 20) for e in (-1, 0, 1)] + [2 ** 63 - 1, 2 ** 63, 2 ** 64 - 2, 2 ** 64 - 1])
DIGIT_POS = [0, 9, 10] + [10 ** d + e for d in range(2, 10) for e in (-1, 0)] + [2 ** 32 - 1]


def digits_sketch():
    """every hash of DIGIT_HASHES with every position of DIGIT_POS, in records of seven entries (and a last one of one): the list
    of hashes is rotated from one position to the next, so that hashes of every length open a line and close one"""
    hashes, pos = [], []
    for j, p in enumerate(DIGIT_POS):
        rot = DIGIT_HASHES[(3 * j) % len(DIGIT_HASHES):] + DIGIT_HASHES[:(3 * j) % len(DIGIT_HASHES)]
        hashes += rot
        pos += [p] * len(rot)
    n = len(hashes)
    record = np.arange(n, dtype=np.uint32) // 7
    ids = [f"d{r}" for r in range(int(record[-1]) + 1)]
    forward = (np.arange(n) * 7 % 3 != 0).astype(np.uint8)
    return np.array(hashes, dtype=np.uint64), np.array(pos, dtype=np.uint32), record, ids, forward


@pytest.mark.parametrize("with_pos,with_strand", [(False, False), (True, False), (False, True), (True, True)])
def test_digits(capfd, tsv_env, tmp_path, with_pos, with_strand):
    """0, 10^d - 1, 10^d, 10^d + 1 for d = 1 .. 19, 2^63 - 1, 2^63, 2^64 - 2, 2^64 - 1 as hashes, each with the positions 0, 9, 10,
    10^d - 1 and 10^d up to 10^9, and 2^32 - 1; all four column layouts"""
    sketch = digits_sketch()
    hashes, pos, record, ids, forward = sketch
    assert len(hashes) == len(DIGIT_HASHES) * len(DIGIT_POS) == 62 * 20
    assert {len(str(h)) for h in DIGIT_HASHES} == set(range(1, 21)) and {len(str(p)) for p in DIGIT_POS} == set(range(1, 11))
    opens = np.flatnonzero(np.diff(record, prepend=np.uint32(2 ** 32 - 1)))
    closes = np.flatnonzero(np.diff(record, append=np.uint32(2 ** 32 - 1)))
    for where in (opens, closes):
        assert {len(str(h)) for h in hashes[where].tolist()} == set(range(1, 21))
    assert 0 < forward.sum() < len(forward)
    got = check_file(capfd, tsv_env, tmp_path, sketch, with_pos, with_strand)
    if with_strand:
        assert b":+" in got and b":-" in got
    if with_pos and not with_strand:   # two fields per entry: read_minimizers refuses them, and so does add_tsv
        with MxEngine(k=32, w=100) as eng:
            with pytest.raises(MxError, match="exactly three"):
                eng.add_tsv("back", 1.0, str(tmp_path / "dev.tsv"))


# ---------------------------------------------------------------------------------------------------------------
# 2. record shapes
# ---------------------------------------------------------------------------------------------------------------
def _ids(n):
    return [f"r{r}" for r in range(n)]


def long_ids_sketch():
    """ids of 1, 255, 256 and 5000 bytes among records with and without minimizers"""
    ids = ["a", "B" * 255, "c", "D" * 256, "e" * 5000, "f", "G" * 255, "h"]
    return random_sketch(41, 230, ids, [0, 40, 1, 0, 90, 0, 99, 0])


RECORD_SHAPES = {
    "nothing-1-record": lambda: random_sketch(1, 0, _ids(1), [0]),
    "nothing-3-records": lambda: random_sketch(1, 0, _ids(3), [0] * 3),
    "nothing-300-records": lambda: random_sketch(1, 0, _ids(300), [0] * 300),
    "empty-first": lambda: random_sketch(2, 30, _ids(5), [0, 0, 10, 5, 15]),
    "empty-last": lambda: random_sketch(3, 30, _ids(5), [10, 5, 15, 0, 0]),
    "empty-row-of-600": lambda: random_sketch(4, 5, _ids(602), [3] + [0] * 600 + [2]),     # (k_tsv_ids: blocks of 256 records)
    "only-row-of-600-then-one": lambda: random_sketch(5, 1, _ids(601), [0] * 600 + [1]),
    "alternating-empty-first": lambda: random_sketch(6, 300, _ids(600), [0, 1] * 300),
    "alternating-empty-last": lambda: random_sketch(7, 300, _ids(600), [1, 0] * 300),
    "id-lengths": long_ids_sketch,
    "one-record": lambda: random_sketch(8, 3000, ["all"], [3000]),
}


@pytest.mark.parametrize("shape", sorted(RECORD_SHAPES))
def test_record_shapes(capfd, tsv_env, tmp_path, shape):
    """no minimizers at all; records without minimizers first, last, 600 in a row, alternating with records of one; ids of 1, 255,
    256 and 5000 bytes; one record that holds everything.  Positions and strands on, so that all of (a), (b), (c) apply"""
    sketch = RECORD_SHAPES[shape]()
    got = check_file(capfd, tsv_env, tmp_path, sketch, True, True)
    assert got.count(b"\n") == len(sketch[3])


# ---------------------------------------------------------------------------------------------------------------
# 3. tiles and passes of the offset scan
# ---------------------------------------------------------------------------------------------------------------
def scan_sketch(n):
    ids = [f"s{r}" if r % 50 else "long-id-" * 40 + str(r) for r in range(300)]
    return random_sketch(n, n, ids)


@pytest.mark.parametrize("n", [1, 255, 256, 257, TILE - 1, TILE, TILE + 1, 4 * TILE + 1])
def test_scan_tile_borders(capfd, tsv_env, tmp_path, n):
    """n on both sides of a block of k_tsv_len (256) and of a scan tile (1024), and a few tiles; 300 records, at least 60 of them
    without minimizers; hash lengths uniform over 1 .. 20 digits, so that no two tile sums agree"""
    check_file(capfd, tsv_env, tmp_path, scan_sketch(n), True, True)


@pytest.mark.parametrize("n,with_pos,with_strand,host", [(PASS - 1, False, False, False), (PASS + 1, False, False, True),
                                                         (PASS, True, True, False), (2 * PASS + 1025, True, False, False)])
def test_scan_pass_borders(capfd, tsv_env, tmp_path, n, with_pos, with_strand, host):
    """n = P - 1, P, P + 1 and 2 P + 1025 for P = 4 194 304, the entries of one pass of k_tsv_scan_tiles: the 64-bit carry from pass
    to pass first matters at P + 1.  Four values of n are four device files, and the host writer's copy is a fifth: more than the
    three files of this size the tests were meant to keep to.  To keep the cases at seconds, only two of them are of several windows: P - 1 and
    P + 1 are written without positions (48 MB: the scan sees the same 4 M lengths, one window), P with positions and strands (its
    file is read back, check (c)), 2 P + 1025 with positions; the host writer's copy, check (b), is made of the P + 1 case only.
    The files of P and of 2 P + 1025 cross one and two real 64 MiB window borders: their sizes are asserted"""
    got = check_file(capfd, tsv_env, tmp_path, scan_sketch(n), with_pos, with_strand, host=host)
    if with_pos:
        assert len(got) > (n // PASS) * WIN, len(got)
    else:
        assert len(got) < WIN


# ---------------------------------------------------------------------------------------------------------------
# 4. window borders
# ---------------------------------------------------------------------------------------------------------------
def window_ids_sketch():
    """ids of 1, 255, 256 and 5000 bytes in front of 600 records without minimizers in a row, between records that have some"""
    ids = ["a", "B" * 255, "c" * 256, "D" * 5000] + _ids(600) + ["z"]
    return random_sketch(9, 400, ids, [100, 1, 0, 150] + [0] * 600 + [149])


WINDOW_FILES = {"digits": digits_sketch, "ids": window_ids_sketch}
WINDOW_SIZES = {"1": lambda total: 1, "2": lambda total: 2, "3": lambda total: 3, "7": lambda total: 7, "64": lambda total: 64,
                "4096": lambda total: 4096, "total-1": lambda total: total - 1, "total": lambda total: total,
                "total+1": lambda total: total + 1}


@pytest.fixture(scope="module")
def default_runs(tmp_path_factory):
    """{name: (the sketch, the bytes the device writer gives with its own 64 MiB windows)}, each checked against the reference"""
    runs = {}
    with pytest.MonkeyPatch.context() as env:
        for name in ("MXG_HOST_TSV", "MXG_TSV_WIN"):
            env.delenv(name, raising=False)
        for name, make in WINDOW_FILES.items():
            sketch = make()
            hashes, pos, record, ids, forward = sketch
            got, sk, knobs = write(None, tmp_path_factory.mktemp("default") / f"{name}.tsv", sketch, True, True)
            assert not [k for k in knobs if k.startswith(("MXG_HOST_TSV", "MXG_TSV_WIN"))]
            same_bytes(got, reference_text(hashes, pos, record, ids, True, True, sk["forward"]), "default run against the reference")
            runs[name] = (sketch, got)
    return runs


@pytest.mark.parametrize("win", list(WINDOW_SIZES))
@pytest.mark.parametrize("name", sorted(WINDOW_FILES))
def test_window_borders(capfd, tsv_env, tmp_path, default_runs, name, win):
    """MXG_TSV_WIN: the digits file (entries of up to 20 + 1 + 10 + 2 bytes: at 7 bytes a window each of them spans four windows or
    more) and a file of long ids and 600 records without minimizers in a row (every id, tab and lone line end meets a border at every
    alignment), positions and strands on, at windows of 1, 2, 3, 7, 64, 4096 bytes and of one byte less than, exactly, and one byte
    more than the file: the bytes of the default run"""
    sketch, want = default_runs[name]
    assert 10_000 < len(want) < 50_000
    size = WINDOW_SIZES[win](len(want))
    tsv_env.setenv("MXG_TSV_WIN", str(size))
    got, _, knobs = write(capfd, tmp_path / "win.tsv", sketch, True, True)
    assert f"MXG_TSV_WIN={size}" in knobs
    same_bytes(got, want, f"windows of {size} bytes against the default run")


def test_window_size_is_clamped(capfd, tsv_env, tmp_path, default_runs):
    """0 means the minimum, 1; anything above 64 MiB means 64 MiB (the device windows do not grow)"""
    sketch, want = default_runs["ids"]
    for size in ("0", str((64 << 20) + 1), str(1 << 40)):
        tsv_env.setenv("MXG_TSV_WIN", size)
        got, _, knobs = write(capfd, tmp_path / "win.tsv", sketch, True, True)
        assert f"MXG_TSV_WIN={size}" in knobs
        same_bytes(got, want, f"MXG_TSV_WIN={size} against the default run")


# ---------------------------------------------------------------------------------------------------------------
# 5. both sides of k = 200
# ---------------------------------------------------------------------------------------------------------------
def _fasta(path):
    rng = random.Random(200)
    seq = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    recs = [("plain", seq(3000)), ("withN", seq(1500) + "N" * 300 + seq(1400)), ("lower", seq(2500).lower()),
            ("short", seq(150)), ("mixed extra words", "".join(c.lower() if rng.random() < 0.3 else c for c in seq(2000)))]
    with open(path, "w") as fh:
        for rid, s in recs:
            fh.write(">" + rid + "\n")
            for p in range(0, len(s), 70):
                fh.write(s[p:p + 70] + "\n")
    return recs


def _sketched_tsv(capfd, fa, k, out, device, with_strand=False):
    capfd.readouterr()
    with MxEngine(k=k, w=10, threads=3) as eng:
        eng.add_fasta("x", 1.0, fa)
        eng.sketch()
        eng.write_tsv(0, out, with_pos=True, with_strand=with_strand, with_seq=True)
        n = eng.stats()["minimizers"]
    assert (DEVICE_LINE in capfd.readouterr().err) == device
    with open(out, "rb") as fh:
        return fh.read(), n


@pytest.mark.parametrize("k", [199, 200, 201, 250])
def test_k_on_both_sides_of_the_route_switch(capfd, tsv_env, tmp_path, oracle, k):
    """write_tsv formats on the device up to k = 200 (an entry's length is kept in one byte: 20 + 1 + 10 + 2 + 1 + 200 + 1 = 235)
    and on the host above; a FASTA with an N run, a lower-case record, a mixed-case one and one shorter than k, against the oracle's
    FASTA -> TSV driver, k-mer column on.  Up to 200 also the host writer, both behind the device parser (it then fetches the text
    from the device to spell the k-mers as the file does) and behind the host parser"""
    fa = str(tmp_path / "k.fa")
    _fasta(fa)
    want = str(tmp_path / "want.tsv")
    oracle.fasta_to_tsv(fa, want, k, 10)
    with open(want, "rb") as fh:
        want = fh.read()
    got, n = _sketched_tsv(capfd, fa, k, str(tmp_path / "dev.tsv"), device=k <= 200)
    assert n > 1000 and re.search(rb":[acgt]{%d}[ \n]" % k, want) and b"short\t\n" in want
    same_bytes(got, want, f"k = {k} against the oracle")
    routes = [{"MXG_HOST_INGEST": "1"}]
    if k <= 200:
        routes += [{"MXG_HOST_TSV": "1"}, {"MXG_HOST_TSV": "1", "MXG_HOST_INGEST": "1"}]
    for env in routes:
        for name, value in env.items():
            tsv_env.setenv(name, value)
        got, _ = _sketched_tsv(capfd, fa, k, str(tmp_path / "host.tsv"), device=False)
        for name in env:
            tsv_env.delenv(name)
        same_bytes(got, want, f"k = {k} with {env} against the oracle")


@pytest.mark.parametrize("k", [32, 200])
def test_strand_column_of_a_sketched_fasta(capfd, tsv_env, tmp_path, oracle, k):
    """with_strand=True on a sketch the kernels made (the strands come from k_strand), k-mer column on, against the oracle"""
    fa = str(tmp_path / "k.fa")
    _fasta(fa)
    want = str(tmp_path / "want.tsv")
    oracle.fasta_to_tsv(fa, want, k, 10, pos=True, strand=True, seq=True)
    with open(want, "rb") as fh:
        want = fh.read()
    assert b":+:" in want and b":-:" in want
    got, _ = _sketched_tsv(capfd, fa, k, str(tmp_path / "dev.tsv"), device=True, with_strand=True)
    same_bytes(got, want, f"strand column at k = {k} against the oracle")
