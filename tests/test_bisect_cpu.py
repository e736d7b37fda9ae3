"""CPU tests of the two bisections every stage shares (ntjoin_amd/csrc/bisect.h: last_where, first_where and their array forms
last_le, first_ge, first_gt), run on the host by tools/bisect_check.cpp, which is built here with the host compiler and decides
nothing: every expected value comes from Python's bisect module."""
import bisect
import os
import random
import shutil
import subprocess

import pytest

from tests.conftest import REPO

CSRC = os.path.join(REPO, "ntjoin_amd", "csrc")
SIZES = [0, 1, 2, 3, 4, 255, 256, 257, 65537]
HIGH = 1 << 32   # the "high" keys lie above it: a comparison of low halves alone would get them wrong


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    out = tmp_path_factory.mktemp("bisect_check") / "bisect_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(REPO, "tools", "bisect_check.cpp"), "-o", str(out)])
    return str(out)


def keys_of(n, pattern):
    rng = random.Random(7000 + n)
    if pattern == "distinct":    # strictly rising, gaps between the keys
        return [3 * i + 5 for i in range(n)]
    if pattern == "runs":        # runs of equal keys of 1 to 5
        out, v = [], 10
        while len(out) < n:
            out += [v] * rng.randint(1, 5)
            v += rng.randint(1, 3)
        return out[:n]
    if pattern == "equal":
        return [77] * n
    assert pattern == "high"     # 64-bit keys above 2^32 whose low halves do not rise
    return sorted(HIGH * rng.randint(1, 1 << 30) + rng.randint(0, HIGH - 1) for _ in range(n))


def queries_of(keys):
    "below every key, above every key, the first key, the last key, keys and their neighbours in between"
    if not keys:
        return [0, 1, (1 << 64) - 1]
    rng = random.Random(len(keys))
    some = [keys[rng.randrange(len(keys))] for _ in range(40)]
    q = [0, keys[0] - 1, keys[0], keys[0] + 1, keys[-1] - 1, keys[-1], keys[-1] + 1, (1 << 64) - 1]
    return q + some + [x - 1 for x in some] + [x + 1 for x in some]


def ranges_of(n):
    "the whole array and, where there is room, a range with lo > 0 and hi < n"
    return [(0, n)] + ([(1, n - 1), (n // 2, n // 2), (n // 2, n // 2 + 1)] if n >= 3 else [])


def run(exe, tmp_path, op, keys, queries, lo, hi):
    import numpy as np
    np.array(keys, dtype=np.uint64).tofile(tmp_path / "k")
    np.array(queries, dtype=np.uint64).tofile(tmp_path / "q")
    r = subprocess.run([exe, op, str(tmp_path / "k"), str(tmp_path / "q"), str(lo), str(hi)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr)
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(rows) == len(queries)
    return rows


@pytest.mark.parametrize("pattern", ["distinct", "runs", "equal", "high"])
@pytest.mark.parametrize("n", SIZES)
def test_owner(exe, tmp_path, n, pattern):
    """the last i in [lo, hi) with keys[i] <= x, and lo where there is none -- keys[lo] is taken for granted: the program's
    predicate ends it with status 4 if it is ever asked about lo"""
    keys = keys_of(n, pattern)
    queries = queries_of(keys)
    for lo, hi in ranges_of(n):
        want = [max(bisect.bisect_right(keys, x, lo, hi) - 1, lo) for x in queries]
        got = run(exe, tmp_path, "owner", keys, queries, lo, hi)
        assert got == [(w, w) for w in want], (lo, hi)


@pytest.mark.parametrize("pattern", ["distinct", "runs", "equal", "high"])
@pytest.mark.parametrize("n", SIZES)
def test_first(exe, tmp_path, n, pattern):
    "the first i in [lo, hi) with keys[i] >= x, and with keys[i] > x; hi where there is none"
    keys = keys_of(n, pattern)
    queries = queries_of(keys)
    for lo, hi in ranges_of(n):
        want = [(bisect.bisect_left(keys, x, lo, hi), bisect.bisect_right(keys, x, lo, hi)) for x in queries]
        assert run(exe, tmp_path, "first", keys, queries, lo, hi) == want, (lo, hi)


WRAP_LO, WRAP_HI = 0x80000000, 0xFFFFFFFF
WRAP_T = [0x80000000, 0x80000001, 0xA0000000, 0xBFFFFFFF, 0xC0000000, 0xC0000001, 0xFFFFFFFE, 0xFFFFFFFF, 0x7FFFFFFF]


def test_midpoint_does_not_wrap(exe):
    """32-bit indices [0x80000000, 0xFFFFFFFF) and the predicate i >= t, which reads no memory.  The midpoint the parent's copies
    computed, (lo + hi) >> 1 in 32 bits, wraps here: lo + hi = 0x17FFFFFFF, of which 32 bits keep 0x7FFFFFFF, and half of that,
    0x3FFFFFFF, lies below lo -- outside the range, where i >= t is false for every t of the range, so that loop would move lo DOWN to
    0x40000000 and go on from there.  lo + ((hi - lo) >> 1) = 0xBFFFFFFF is the true midpoint."""
    wrapped = ((WRAP_LO + WRAP_HI) & 0xFFFFFFFF) >> 1
    assert WRAP_LO + WRAP_HI >= 1 << 32 and wrapped == 0x3FFFFFFF < WRAP_LO
    assert WRAP_LO + ((WRAP_HI - WRAP_LO) >> 1) == (WRAP_LO + WRAP_HI) >> 1 == 0xBFFFFFFF
    r = subprocess.run([exe, "wrap", hex(WRAP_LO), hex(WRAP_HI)] + [hex(t) for t in WRAP_T], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    # the first i of the range with i >= t: t itself inside the range, lo for a t below it, hi for t = hi
    want = [min(max(t, WRAP_LO), WRAP_HI) for t in WRAP_T]
    assert [int(x) for x in r.stdout.split()] == want
