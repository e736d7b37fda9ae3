"""GPU tests of the shared primitives by themselves -- launch_scan_u32 and count_publish / count_prefix (csrc/scan_kernels.h),
launch_scan_u64 and launch_max_scan_u64 (csrc/scan64_kernels.h), launch_radix_sort (csrc/sort_kernels.h) -- past the borders where
their carry code starts:

  * scan32 around the tile (1024), one pass of k_scan_sums (4096 tiles = 4 194 304 inputs) and two passes, with prefixes that pass
    2^32, and `total` on both sides of the limit the header states;
  * scan64 around the tile, one round of k_pt_scan_tiles (256 tiles = 262 144 inputs) and two rounds, with prefixes past 2^32;
  * maxscan64, the running 64-bit maximum, around the block, the tile, one round of k_pt_max_tiles (262 144 inputs) and two rounds
    plus one, against np.maximum.accumulate: rising (the output is the input), falling (every output lives on a carry), one value
    among zeros on either side of a tile and of a round border, the callers' (record << 32) | x, words with the top bit set, zeros;
  * the sort around the wave, the round, the tile and past 2^16, with odd and even pass counts, against numpy's stable argsort bit
    for bit (values = indices, so every place of every equal key is checked: the direct test of its stability), and once with more
    than 16 384 tiles, where the scan over its counts takes a second pass;
  * count_prefix around the super-count (256 producer blocks), the first lanes' own loads (16 384), and the first and second trip of
    the loop over the super-counts (16 640, 82 176);
  * the two bisections of csrc/bisect.h over 1 to 65 537 keys with runs of equal ones and keys above 2^32, one thread per query with a
    partial last block, once over 32-bit indices where (lo + hi) >> 1 would wrap; the device writers' one window-bounds kernel
    (launch_win_bounds, win_out.hip) with windows of 1 byte, 4093 bytes and exactly one line, on and one byte before an offset;
  * one run of the public API -- build_graph, synteny_blocks, write_synteny_paf, synteny_assess -- on 4 456 499 anchors in 262 147
    blocks (tests/_synteny_scale.py), past both scan borders, against the closed form and the restatements.

ntjoin_amd/bin/prim_check (tools/prim_check.hip) runs one primitive once on arrays from files, every device array at exactly its
documented size between guard bytes, and decides nothing: every expected value is computed here.  One child process per case."""
import os
import subprocess
import time

import numpy as np
import pytest

from tests import _maxscan_model as MM

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "ntjoin_amd", "bin", "prim_check")
PASS32 = 4096 * 1024   # inputs per pass of k_scan_sums
U32 = 1 << 32


def run(*args):
    assert os.path.exists(EXE), "ntjoin_amd/bin/prim_check missing: run __graft_entry__.build()"
    r = subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "guards: ok" in r.stdout, r.stdout + r.stderr
    return r.stdout


def same(got, want, what):
    "equal arrays, or the first place where they differ"
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, the first at [{bad[0]}]: got {got[bad[0]]}, expected {want[bad[0]]}"


# ---- scan32 ------------------------------------------------------------------------------------------------------------------------
SCAN32_SIZES = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, PASS32 - 1, PASS32, PASS32 + 1, 2 * PASS32 + 1]


def scan32_input(n, pattern):
    rng = np.random.default_rng(1000 + n)
    if pattern == "ones":        # the prefix is the index: a failure names the first wrong place
        return np.ones(n, dtype=np.uint32)
    if pattern == "below16":
        return rng.integers(0, 16, n, dtype=np.uint32)
    if pattern == "single":      # zeros and one value, at the last element of the first pass, else of the last whole tile, else of the input
        a = np.zeros(n, dtype=np.uint32)
        a[PASS32 - 1 if n >= PASS32 else n // 1024 * 1024 - 1 if n >= 1024 else n - 1] = 0xFFFFFFF0
        return a
    if pattern == "below1200":   # two passes of about 2.5e9 each: no pass reaches 2^32, their sum does
        return rng.integers(0, 1200, n, dtype=np.uint32)
    assert pattern == "below2p20"   # at the large sizes every pass sums to about 2^41
    return rng.integers(0, 1 << 20, n, dtype=np.uint32)


def total32(a):
    "`total` as scan_kernels.h states it: the sum over the aligned runs of 4 194 304 inputs of (the run's sum mod 2^32)"
    return sum(int(a[lo:lo + PASS32].sum(dtype=np.uint64)) % U32 for lo in range(0, len(a), PASS32))


# (below1200: the exact side of the total's limit past 2^32 needs two whole passes: one size)
SCAN32_CASES = [(n, pattern) for pattern in ("ones", "below16", "single", "below2p20") for n in SCAN32_SIZES] + [(2 * PASS32 + 1, "below1200")]


@pytest.mark.parametrize("n,pattern", SCAN32_CASES)
def test_scan32(n, pattern, tmp_path):
    a = scan32_input(n, pattern)
    a.tofile(tmp_path / "in")
    run("scan32", tmp_path / "in", tmp_path / "out", tmp_path / "total")
    incl = np.cumsum(a, dtype=np.uint64)
    same(np.fromfile(tmp_path / "out", dtype=np.uint32), ((incl - a) & np.uint64(U32 - 1)).astype(np.uint32), f"scan32 {n} {pattern}")
    total, exact = int(np.fromfile(tmp_path / "total", dtype=np.uint64)[0]), int(incl[-1])
    assert total == total32(a), (total, total32(a), exact)
    # both sides of the limit: exact while every run of 4 194 304 inputs sums below 2^32 (past 2^32 as a whole, too), not beyond
    if pattern == "below1200":
        assert total == exact > U32
    elif pattern == "below2p20" and n >= PASS32 - 1:
        assert exact > U32 and total != exact and total < 3 * U32
    else:
        assert total == exact


# ---- scan64 ------------------------------------------------------------------------------------------------------------------------
SCAN64_SIZES = [1, 2, 255, 256, 257, 1023, 1024, 1025, 262143, 262144, 262145, 524289]


def scan64_input(n, pattern):
    rng = np.random.default_rng(2000 + n)
    if pattern == "ones":
        return np.ones(n, dtype=np.uint64)
    if pattern == "below2p40":   # prefixes pass 2^32 at once: byte offsets of a file beyond 4 GB
        return rng.integers(0, 1 << 40, n, dtype=np.uint64)
    if pattern == "one2p62":     # one value of 2^62 in the first tile among small ones
        a = rng.integers(0, 100, n, dtype=np.uint64)
        a[min(n - 1, 700)] = 1 << 62
        return a
    assert pattern == "total_at_n"   # the callers' idiom: n + 1 entries, the last one 0, the total is read at [n]
    a = rng.integers(0, 1 << 33, n + 1, dtype=np.uint64)
    a[n] = 0
    return a


@pytest.mark.parametrize("pattern", ["ones", "below2p40", "one2p62", "total_at_n"])
@pytest.mark.parametrize("n", SCAN64_SIZES)
def test_scan64(n, pattern, tmp_path):
    a = scan64_input(n, pattern)
    assert sum(a.tolist()) < 1 << 64
    a.tofile(tmp_path / "in")
    run("scan64", tmp_path / "in", tmp_path / "out")
    got = np.fromfile(tmp_path / "out", dtype=np.uint64)
    same(got, np.cumsum(a, dtype=np.uint64) - a, f"scan64 {n} {pattern}")
    if pattern == "total_at_n":
        assert int(got[n]) == sum(a.tolist())


# ---- maxscan64 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,pattern,at", MM.cases(), ids=lambda v: "" if v is None else str(v))
def test_maxscan64(n, pattern, at, tmp_path):
    """the inputs are tests/_maxscan_model.py's, which says what each pattern is there for; tests/test_maxscan_model_cpu.py shows that
    each would come out wrong under the carry faults it names"""
    a = MM.pattern_input(n, pattern, at)
    a.tofile(tmp_path / "in")
    run("maxscan64", tmp_path / "in", tmp_path / "out")
    same(np.fromfile(tmp_path / "out", dtype=np.uint64), np.maximum.accumulate(a), f"maxscan64 {n} {pattern} {at}")


# ---- sort --------------------------------------------------------------------------------------------------------------------------
SORT_SIZES = [2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 65537]
SORT_PATTERNS = ["seeded", "three", "equal", "sorted", "reversed", "tail_digit0", "high_bits"]
KEY_BITS = [8, 9, 16, 33, 40, 64]
SORT_BIG = 16 * 1024 * 1024 + 1   # 16 385 tiles: 4 194 560 counts, a second pass of k_scan_sums inside the sort


def sort_keys(n, key_bits, pattern):
    rng = np.random.default_rng(3000 + n + key_bits)
    top = (1 << key_bits) - 1
    seeded = rng.integers(0, top, n, dtype=np.uint64, endpoint=True)
    if pattern == "seeded":       # over the full width of the key
        return seeded
    if pattern == "three":        # long runs of equal keys across wave, round and tile borders
        return np.array([0, top // 2 + 1, top], dtype=np.uint64)[rng.integers(0, 3, n)]
    if pattern == "equal":
        return np.full(n, top // 3, dtype=np.uint64)
    if pattern == "sorted":
        return np.sort(seeded)
    if pattern == "reversed":
        return np.sort(seeded)[::-1].copy()
    if pattern == "tail_digit0":  # the last tile's (below a tile: the last round's) real keys have digit 0 in every pass, as its idle lanes do
        seeded[(n - 1) // 1024 * 1024 if n > 1024 else (n - 1) // 64 * 64:] = 0
        return seeded
    assert pattern == "high_bits"  # the documented precondition: the bits above key_bits are the same in every key, here not 0
    return seeded | np.uint64((1 << 63) | (0x5A5A << 44 if key_bits <= 40 else 0))


def check_sort(n, key_bits, keys, tmp_path):
    vals = np.arange(n, dtype=np.uint32)
    keys.tofile(tmp_path / "k")
    vals.tofile(tmp_path / "v")
    out = run("sort", key_bits, tmp_path / "k", tmp_path / "v", tmp_path / "ko", tmp_path / "vo")
    passes = (key_bits + 7) // 8
    assert f"buffer: {passes & 1 if n >= 2 else 0}\n" in out, out
    masked = keys & np.uint64((1 << key_bits) - 1)
    order = np.argsort(masked.astype(np.uint16) if key_bits <= 16 else masked, kind="stable")
    same(np.fromfile(tmp_path / "vo", dtype=np.uint32), order.astype(np.uint32), f"sort {n} {key_bits} values")
    same(np.fromfile(tmp_path / "ko", dtype=np.uint64), keys[order], f"sort {n} {key_bits} keys")


@pytest.mark.parametrize("pattern", SORT_PATTERNS)
@pytest.mark.parametrize("n", SORT_SIZES)
def test_sort(n, pattern, tmp_path):
    "every size with every pattern; the key widths go round, so that every pattern and every size meets each of them"
    key_bits = KEY_BITS[(SORT_SIZES.index(n) + SORT_PATTERNS.index(pattern)) % len(KEY_BITS)]
    check_sort(n, key_bits, sort_keys(n, key_bits, pattern), tmp_path)


@pytest.mark.parametrize("key_bits", KEY_BITS)
@pytest.mark.parametrize("n", [0, 1])
def test_sort_of_nothing_and_of_one(n, key_bits, tmp_path):
    "returns 0 and launches nothing: the pair stays where it was"
    check_sort(n, key_bits, sort_keys(n, key_bits, "seeded"), tmp_path)


@pytest.mark.parametrize("pattern", ["seeded", "three"])
def test_sort_past_16384_tiles(pattern, tmp_path):
    t0 = time.time()
    check_sort(SORT_BIG, 16, sort_keys(SORT_BIG, 16, pattern), tmp_path)
    print(f"sort of {SORT_BIG} pairs, key_bits 16, {pattern}: {time.time() - t0:.1f} s")


# ---- count_publish / count_prefix --------------------------------------------------------------------------------------------------
PREFIX_SIZES = [0, 1, 255, 256, 257, 16383, 16384, 16385, 16639, 16640, 16641, 82175, 82176, 82177, 200000]


@pytest.mark.parametrize("more", [0, 300])
@pytest.mark.parametrize("q", PREFIX_SIZES)
def test_count_prefix(q, more, tmp_path):
    "q of q + more producer blocks: what the blocks from q on published (into cnt and into the last super-counts) is not counted"
    rng = np.random.default_rng(4000 + q)
    counts = rng.integers(0, 5000, q + more, dtype=np.uint32)
    counts[rng.random(q + more) < 0.3] = 0
    assert int(counts.sum(dtype=np.uint64)) < U32
    counts.tofile(tmp_path / "c")
    out = run("prefix", q, tmp_path / "c")
    assert f"prefix: {int(counts[:q].sum(dtype=np.uint64))}\n" in out, out


# ---- the bisections (csrc/bisect.h) and the window-bounds kernel every device writer shares (win_out.hip) ---------------------------
BISECT_N = [1, 2, 3, 64, 65, 256, 257, 65537]
BISECT_NQ = [1, 255, 256, 257]   # one thread per query: a lone thread, a block less one, a whole block, a block and one thread
# every n with one query count, the counts going round; the smallest odd n and the largest with every count
BISECT_CASES = sorted({(n, BISECT_NQ[i % 4]) for i, n in enumerate(BISECT_N)} | {(n, nq) for n in (3, 65537) for nq in BISECT_NQ})


def bisect_input(n, nq):
    "rising keys with runs of equal ones, the upper half of them above 2^32; queries on, beside, below and above the keys"
    rng = np.random.default_rng(5000 + n + nq)
    reps = rng.integers(1, 4, n)
    reps[0] = 2   # (a run of two at the front whenever n >= 3)
    keys = np.repeat(np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(5), reps)[:n]
    keys[(n + 1) // 2:] += np.uint64(1 << 40)
    fixed = [0, int(keys[0]) - 1, int(keys[0]), int(keys[-1]), int(keys[-1]) + 1, (1 << 64) - 1]
    picks = [int(keys[i]) + d for i, d in zip(rng.integers(0, n, nq).tolist(), rng.integers(-1, 2, nq).tolist())]
    queries = np.array((picks[:max(nq - len(fixed), 1)] + fixed)[:nq], dtype=np.uint64)
    assert len(queries) == nq and (n < 3 or keys[0] == keys[1]) and (np.diff(keys.astype(object)) >= 0).all()
    return keys, queries


@pytest.mark.parametrize("n,nq", BISECT_CASES)
def test_bisect_owner(n, nq, tmp_path):
    "last_le: the last key <= x (0 where every key is above x; keys[0] is never read)"
    keys, queries = bisect_input(n, nq)
    keys.tofile(tmp_path / "k")
    queries.tofile(tmp_path / "q")
    run("owner", tmp_path / "k", tmp_path / "q", tmp_path / "out")
    want = np.maximum(np.searchsorted(keys, queries, side="right").astype(np.int64) - 1, 0)
    same(np.fromfile(tmp_path / "out", dtype=np.uint32).astype(np.int64), want, f"owner {n} {nq}")


@pytest.mark.parametrize("n,nq", BISECT_CASES)
def test_bisect_first(n, nq, tmp_path):
    "first_ge and first_gt: the first key >= x and the first key > x (n where there is none)"
    keys, queries = bisect_input(n, nq)
    keys.tofile(tmp_path / "k")
    queries.tofile(tmp_path / "q")
    run("first", tmp_path / "k", tmp_path / "q", tmp_path / "out")
    got = np.fromfile(tmp_path / "out", dtype=np.uint32).astype(np.int64)
    same(got[:nq], np.searchsorted(keys, queries, side="left").astype(np.int64), f"first_ge {n} {nq}")
    same(got[nq:], np.searchsorted(keys, queries, side="right").astype(np.int64), f"first_gt {n} {nq}")


def test_bisect_midpoint_does_not_wrap(tmp_path):
    """tests/test_bisect_cpu.py's case on the device: 32-bit indices [0x80000000, 0xFFFFFFFF), where (lo + hi) >> 1 in 32 bits is
    0x3FFFFFFF, below lo, and the predicate i >= t reads no memory"""
    lo, hi = 0x80000000, 0xFFFFFFFF
    assert ((lo + hi) & 0xFFFFFFFF) >> 1 == 0x3FFFFFFF < lo
    t = np.array([0x80000000, 0x80000001, 0xA0000000, 0xBFFFFFFF, 0xC0000000, 0xC0000001, 0xFFFFFFFE, 0xFFFFFFFF, 0x7FFFFFFF], dtype=np.uint32)
    t.tofile(tmp_path / "t")
    run("wrap", lo, hi, tmp_path / "t", tmp_path / "out")
    same(np.fromfile(tmp_path / "out", dtype=np.uint32), np.clip(t, lo, hi).astype(np.uint32), "wrap")


def winbounds_input(kind, n_win):
    """the offsets of the items' texts (off[0] = 0, off[n] = the file's size) and the window for n_win windows:
    one_byte  windows of 1 byte over lines of 0 to 3 bytes (items without text share their successor's offset);
    w4093     windows of 4093 bytes over lines of about 60: no window border is a line border but by chance;
    one_line  every line as long as the window: every window starts exactly on an offset;
    borders   windows of 100 bytes; window c starts exactly on an offset for odd c and one byte before one for even c"""
    rng = np.random.default_rng(6000 + n_win)
    if kind == "one_byte":
        win, lens = 1, rng.integers(0, 4, 2 * n_win)
    elif kind == "w4093":
        win, lens = 4093, rng.integers(1, 120, 80 * n_win)
    elif kind == "one_line":
        win, lens = 61, np.full(n_win, 61)
    else:
        assert kind == "borders"
        win = 100
        marks = sorted({c * win + (0 if c & 1 else 1) for c in range(1, n_win)} | {c * win + 37 for c in range(n_win)} | {n_win * win})
        return np.array([0] + marks, dtype=np.uint64), win
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    if kind != "one_line":   # cut to a size of n_win windows, the last of them of one byte
        total = (n_win - 1) * win + 1
        off = np.concatenate([off[off < total], [total]]).astype(np.uint64)
    return off, win


@pytest.mark.parametrize("n_win", [1, 256, 257])
@pytest.mark.parametrize("kind", ["one_byte", "w4093", "one_line", "borders"])
def test_win_bounds(kind, n_win, tmp_path):
    "bounds[c] = the last item whose text starts at or before byte c * win"
    off, win = winbounds_input(kind, n_win)
    n, total = len(off) - 1, int(off[-1])
    assert off[0] == 0 and (np.diff(off.astype(np.int64)) >= 0).all() and (total + win - 1) // win == n_win
    targets = np.arange(n_win, dtype=np.uint64) * np.uint64(win)
    if kind == "borders" and n_win > 2:
        assert np.isin(targets[1::2], off).all() and np.isin(targets[2::2] + np.uint64(1), off).all() and not np.isin(targets[2::2], off).any()
    off.tofile(tmp_path / "off")
    run("winbounds", tmp_path / "off", win, tmp_path / "out")
    want = np.searchsorted(off[:n], targets, side="right").astype(np.int64) - 1
    same(np.fromfile(tmp_path / "out", dtype=np.uint32).astype(np.int64), want, f"winbounds {kind} {n_win}")


# ---- one stage-level run past both scan borders ------------------------------------------------------------------------------------
def test_synteny_of_262147_blocks(tmp_path):
    """4 456 499 vertices (> 4 194 304: the scans of synteny_blocks over the anchors take a second pass of k_scan_sums), 262 147 kept
    blocks (the PAF writer's line offsets and the assessment's chain lengths: 64-bit scans over 262 148 entries, a second round of
    k_pt_scan_tiles; the assessment's sort of 262 147 chains) through the public API, so with the scratch sizes the stages compute"""
    from ntjoin_amd.engine import MxEngine
    from tests import _assess_restatement as A, _synteny_restatement as R, _synteny_scale as SC
    from tests.test_gpu_assess import SCALARS
    t0 = time.time()
    B = 262147
    case = SC.scale_case(B)
    assert case["n_anchors_total"] == 4456499 > PASS32 and B + 1 > 262144
    with MxEngine(k=case["k"], w=10) as eng:
        for a, asm in enumerate(case["asms"]):
            eng.add_minimizers(f"asm{a}", 1.0, asm["hash"], asm["pos"], asm["record"], asm["names"])
        eng.build_graph()
        got = eng.synteny_blocks(1, 0, max_gap=case["max_gap"], min_anchors=case["min_anchors"], query_length=case["lengths"][1],
                                 subject_length=case["lengths"][0])
        assert (got["n_anchors_total"], got["n_links"], got["n_blocks"]) == (case["n_anchors_total"], case["n_links"], B)
        for name in R.FIELDS:
            same(got[name].astype(np.int64), case["expect"][name].astype(np.int64), name)
        blocks = list(zip(*[got[name].tolist() for name in R.FIELDS]))
        eng.write_synteny_paf(tmp_path / "out.paf")
        q_len, s_len = case["lengths"][1].tolist(), case["lengths"][0].tolist()
        want_paf = R.paf(blocks, SC.QUERY_NAMES, q_len, SC.SUBJECT_NAMES, s_len, case["k"]).encode("ascii")
        assert (tmp_path / "out.paf").read_bytes() == want_paf and want_paf.count(b"\n") == B
        res = eng.synteny_assess(merge_gap=100)   # (below the 160 between two blocks: a chain per block)
        want = A.assess(blocks, case["k"], q_len, s_len, merge_gap=100)
        assert want["n_chains"] == B
        for key in SCALARS:
            assert res[key] == want[key], (key, res[key], want[key])
        for name in A.CHAIN_FIELDS:
            same(res["chains"][name].astype(np.int64), np.array(want["chains"][name], dtype=np.int64), "chain " + name)
        for name in A.BP_FIELDS:
            same(res["bps"][name].astype(np.int64), np.array(want["bps"][name], dtype=np.int64), "breakpoint " + name)
    print(f"synteny of {case['n_anchors_total']} anchors in {B} blocks, PAF and assessment: {time.time() - t0:.1f} s")
