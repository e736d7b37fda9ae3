"""The shipped stream of the bit-sliced ring filter (ntjoin_amd/csrc/gen/bs_gen.py) leaves out ring terms that no test reads; the
generator can also take the wrap test as a carry into the adder (carry_in: fewer instructions and a narrower accept set, [-1, tt]
instead of [-2, tt]; measured and not shipped, profiles/r10/filter_liveness_ab.txt).  Checked on the CPU, with the generator's
numpy VM, for both streams:

  * the VM against `reference_bits` at thresholds on both sides of every special case of the compare (0, 1, a usual one, and the
    three largest: from 2^b - 2 on every sum passes), on chunk 0 (the word in front of it), a middle and the last chunk, on
    inputs where a missing or doubled term shows: random bases, all-A, all-T, a period-31 and a period-32 repeat, a single
    differing base at strip positions 0, 15, 16, 31, at a lane's first and last base and in the strip in front of lane 0.  The ring
    registers hold junk when a chunk begins (what the chunk before and the transposes leave there): the first term a register
    receives must write it;
  * the accept sets: `reference_bits` is [-2, tt], with carry_in [-1, tt], on the sums of a ring recurrence written out here; the
    narrower set lies inside the other and still holds every k-mer whose oracle hash is < tau at the library's thresholds;
  * the generator options alone and combined with the others: 'allterms' (every term made) gives the same bitmap, carry_in the
    set [-1, tt];
  * the instruction counts of the streams and the table of reads that the liveness is derived from.
"""
import functools
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ntjoin_amd", "csrc", "gen"))
import bs_gen as G  # noqa: E402

B = G.B_PLANES
TOP = (1 << B) - 1
N_CHUNKS = 3
LANE = 1024          # base positions per lane: 32 strips of 32
VALU = ("xor", "and", "or", "mov", "bitop3", "add", "lshr", "perm")
THRESHOLDS = (0, 1, 164, TOP - 2, TOP - 1, TOP)


def _edge_codes():
    """three chunks of base codes; in every chunk lanes 0-3 and 60-63 all-A, 4-7 all-T, 8-11 a period-31 and 12-15 a period-32
    repeat, the rest random; single differing bases (each more than 32 positions from the next) in the all-A and all-T lanes;
    one in the last strip of chunks 0 and 1, which is the strip in front of lane 0 of the chunk behind (first / second half)"""
    rng = np.random.default_rng(20240)
    codes = rng.integers(0, 4, N_CHUNKS * G.CHUNK).astype(np.uint8)
    for c in range(N_CHUNKS):
        base = c * G.CHUNK
        codes[base: base + 4 * LANE] = 0
        codes[base + 4 * LANE: base + 8 * LANE] = 3
        codes[base + 8 * LANE: base + 12 * LANE] = np.resize(rng.integers(0, 4, 31), 4 * LANE)
        codes[base + 12 * LANE: base + 16 * LANE] = np.resize(rng.integers(0, 4, 32), 4 * LANE)
        codes[base + 60 * LANE: base + 64 * LANE] = 0
        for bg, lane in ((0, 1), (3, 5)):
            at = base + lane * LANE
            for strip, pos, d in ((3, 0, 1), (9, 15, 2), (15, 16, 3), (21, 31, 1)):
                codes[at + 32 * strip + pos] = (bg + d) % 4
            codes[at + LANE] = (bg + 2) % 4                 # the next lane's first base ...
            codes[at + 2 * LANE - 1] = (bg + 3) % 4         # ... and its last one
        if c < N_CHUNKS - 1:
            codes[base + G.CHUNK - 32 + (5 if c == 0 else 27)] = 2
    return codes


CODES = _edge_codes()
PACKED = G.pack_chunks(CODES, N_CHUNKS)
EXT = np.concatenate([CODES, np.zeros(31, dtype=np.uint8)])   # (bases behind the assembly read as A)


@functools.lru_cache(maxsize=None)
def _gen(ablate=(), perm16=(), lds16=(), carry_in=False):
    g = G.Gen(32, ablate=ablate, perm16=perm16, lds16=lds16, carry_in=carry_in)
    g.chunk()
    return g


@functools.lru_cache(maxsize=None)
def _reference(tt, carry_in=False):
    ref = G.reference_bits(EXT, 32, tt, carry_in=carry_in)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _ring_sums():
    """St of every position of EXT by the rolling recurrence (plane_funcs' docstring), not by reference_bits' direct formula:
    F' = rotl(F) ^ rotl^k(S[out]) ^ S[in],  R' = rotr(R ^ S[3 - out] ^ rotl^k(S[3 - in])) on the top 31 bits of the seeds"""
    k = 32
    S = [G.top31(x) for x in G.SEED]
    Sk = [G.rotl31(x, k) for x in S]
    codes = EXT.tolist()
    F = R = 0
    for j in range(k):
        F = G.rotl31(F, 1) ^ S[codes[j]]
        R ^= G.rotl31(S[3 - codes[j]], j)
    n = len(codes) - k + 1
    St = np.empty(n, dtype=np.int64)
    low = 31 - B
    for p in range(n):
        St[p] = ((F >> low) + (R >> low)) & TOP
        if p + 1 < n:
            o, i = codes[p], codes[p + k]
            F = G.rotl31(F, 1) ^ Sk[o] ^ S[i]
            R = G.rotl31(R ^ S[3 - o] ^ Sk[3 - i], 30)
    St.setflags(write=False)
    return St


def _wide_set(tt):
    """St in [-2, tt] mod 2^b"""
    St = _ring_sums()
    return (St <= tt) | (St >= TOP - 1)


def _narrow_set(tt):
    """St in [-1, tt] mod 2^b; every St from tt = 2^b - 2 on"""
    St = _ring_sums()
    return np.ones(len(St), dtype=bool) if tt >= TOP - 1 else (St <= tt) | (St == TOP)


def _words(bits, c):
    """the 2048 words that chunk c writes, [c * 2048 - 1, c * 2048 + 2047) of the position bitmap (in front of chunk 0: none)"""
    w = (bits[:N_CHUNKS * G.CHUNK].reshape(-1, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1)
    lo = c * 2048 - 1
    return w[max(lo, 0): lo + 2048], (1 if lo < 0 else 0)


def _run_vm(g, tt, c):
    vm = G.VM(PACKED, tt, c, min(c + 1, N_CHUNKS - 1))
    junk = np.random.default_rng(1000 * c + tt)
    for reg in g.FP + g.RP + [g.le, g.ones, g.s, g.cy] + g.M:   # what the chunk before left in them
        vm.vr[reg] = junk.integers(0, 1 << 32, 64, dtype=np.uint64).astype(np.uint32)
    return np.asarray(vm.run(g)[:2048], dtype=np.uint64)


def _assert_bitmap(g, tt, c, bits):
    want, first = _words(bits, c)
    got = _run_vm(g, tt, c)[first:]
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (tt, c, bad[:5].tolist(), [(hex(int(got[i])), hex(int(want[i]))) for i in bad[:5]])


@pytest.mark.parametrize("c", [0, 1, 2])
@pytest.mark.parametrize("tt", THRESHOLDS)
@pytest.mark.parametrize("carry_in", [False, True])
def test_vm_matches_reference_bits_on_edge_inputs(carry_in, tt, c):
    _assert_bitmap(_gen(carry_in=carry_in), tt, c, _reference(tt, carry_in))


def test_the_edge_inputs_decide_something():
    """at the usual threshold the all-A / all-T / periodic lanes and the single bases make both outcomes, so a wrong term in
    them would show; at the three largest thresholds the densities are what the set says"""
    for carry_in in (False, True):
        ref = _reference(164, carry_in)
        for lo, hi in ((0, 4), (4, 8), (8, 12), (12, 16)):
            part = np.concatenate([ref[c * G.CHUNK + lo * LANE: c * G.CHUNK + hi * LANE] for c in range(N_CHUNKS)])
            assert 0 < part.sum() < part.size, (lo, hi)
        assert _reference(TOP, carry_in).all() and _reference(TOP - 1, carry_in).all()
    assert _reference(TOP - 2).all()                # [-2, 2^b - 3] is every sum
    assert not _reference(TOP - 2, True).all()      # St = 2^b - 2 alone fails: [-1, 2^b - 3]


@pytest.mark.parametrize("tt", THRESHOLDS + (40,))
def test_references_are_the_stated_sets_one_inside_the_other(tt):
    St = _ring_sums()
    wide, narrow = _reference(tt), _reference(tt, True)
    assert np.array_equal(wide, _wide_set(tt))
    assert np.array_equal(narrow, _narrow_set(tt))
    assert not (narrow & ~wide).any()
    assert np.array_equal(wide & ~narrow, (St == TOP - 1) & (tt < TOP - 1))   # what carry_in no longer lets through: St = -2


@pytest.mark.parametrize("cand_per_window,w", [(2, 1000), (8, 1000), (18, 500)])
def test_both_references_are_supersets_of_the_oracle(oracle, cand_per_window, w):
    """tau as the library sets it (sparse_plan: tau_hi = even(frac * 2^32), tau = tau_hi << 32; bs_hash: T = tau_hi / 2,
    tt = (T - 1) >> (31 - planes)): every k-mer with hash < tau passes"""
    rng = np.random.default_rng(cand_per_window * 1000 + w)
    codes = rng.integers(0, 4, 400_000).astype(np.uint8)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[codes].tobytes()
    mh, _, _, ok = oracle.kmer_hashes(seq, 32)
    assert ok.all()
    tau_hi = max(2, int(min(4294967294.0, cand_per_window / w * 4294967296.0)) & ~1)
    tt = ((tau_hi >> 1) - 1) >> (31 - B)
    narrow, wide = G.reference_bits(codes, 32, tt, carry_in=True), G.reference_bits(codes, 32, tt)
    real = mh < np.uint64(tau_hi << 32)
    assert real.sum() > 100
    assert not (real & ~narrow).any() and not (narrow & ~wide).any()


@pytest.mark.parametrize("kw", [
    {"ablate": ("allterms",)}, {"carry_in": True}, {"ablate": ("allterms",), "carry_in": True},
    {"ablate": ("nowarmpairs",)}, {"ablate": ("nowarmpairs", "allterms")}, {"ablate": ("nowarmpairs",), "carry_in": True},
    {"ablate": ("nowarmpairs", "allterms"), "carry_in": True},
    {"perm16": ("in", "out")}, {"lds16": ("in", "out")}, {"perm16": ("in", "out"), "ablate": ("allterms",), "carry_in": True}])
@pytest.mark.parametrize("tt", [1, 164, TOP - 2])
def test_generator_options_alone_and_combined(kw, tt):
    """'allterms' (every ring term made, read or not): the bitmap of the default stream; carry_in: the set [-1, tt] -- with one or
    two warm-up steps per pass and with the transposes' other forms"""
    g = _gen(**kw)
    carry_in = kw.get("carry_in", False)
    bits = _narrow_set(tt) if carry_in else _wide_set(tt)
    for c in (0, 1):
        _assert_bitmap(g, tt, c, bits)
    assert g.kernel_tt(tt) == (min(tt + 1, TOP) if carry_in else tt)


def _n_valu(g):
    return sum(1 for i in g.ins if i[0] in VALU)


def test_instruction_counts():
    """the stream of the round before has 7840 instructions; the dead ring terms are 491 of them (the shipped stream), the wrap
    test as a carry-in takes 32 x 15 more (both together: the 6901 the change was planned with, and the first compare's own
    initial value, 32)"""
    g, both = _gen(), _gen(carry_in=True)
    assert _n_valu(_gen(ablate=("allterms",))) == 7840
    assert _n_valu(g) == 7840 - 491
    assert _n_valu(_gen(ablate=("allterms",), carry_in=True)) == 7840 - 32 * 15
    assert _n_valu(both) == 7840 - 491 - 32 * 15 <= 6901
    assert sum(1 for i in g.ins if i[0] == "bitop3") <= 3164 and sum(1 for i in both.ins if i[0] == "bitop3") <= 3164
    g.check_banks()
    both.check_banks()
    assert not any(i[0] in ("mov", "and", "or") and both.ones in i[1:] for i in both.ins)   # no all-ones chain
    inc = open(os.path.join(REPO, "ntjoin_amd", "csrc", "hash_bs_k32.inc")).read()
    assert f"#define HASH_BS_VALU_PER_CHUNK {_n_valu(g)}\n" in inc and "#define HASH_BS_CARRY_IN 0 " in inc


def test_reads_table_is_what_the_tests_read():
    """the table the liveness is derived from, against the stream itself: the adder instructions of productive step t (those
    that write the sum plane) read exactly the registers whose entry holds t"""
    g = _gen(ablate=("allterms",), carry_in=True)     # (the carry-in's lowest plane has a truth table of its own)
    rf, rr = g.reads()
    assert all(rf[r] and rr[r] for r in range(G.RING))
    assert sum(len(x) for x in rf) == sum(len(x) for x in rr) == 32 * B
    seen_f = [set() for _ in range(G.RING)]
    seen_r = [set() for _ in range(G.RING)]
    lowest = {g.tt3(lambda a, b, c: a ^ b ^ 1, x, y, 0) for x in (0, 1) for y in (0, 1)}   # (no carry among its sources)
    t = -1
    for ins in g.ins:
        if ins[0] == "bitop3" and ins[1] == g.s:
            if ins[5] in lowest:
                t += 1     # the lowest plane opens a step
            seen_f[g.FP.index(ins[2])].add(t)
            seen_r[g.RP.index(ins[3])].add(t)
    assert t == 31
    assert seen_f == rf and seen_r == rr


@pytest.mark.parametrize("carry_in", [False, True])
def test_every_register_is_written_before_it_is_read(carry_in):
    """with the dead terms left out: per ring register, the first instruction that names it writes it without reading it"""
    g = _gen(carry_in=carry_in)
    ring = set(g.FP + g.RP)
    first_test = next(i for i, ins in enumerate(g.ins) if ins[0] == "bitop3" and ins[1] == g.s)
    start = next(i for i, ins in enumerate(g.ins) if ins[0] == "prev_stores")   # (before it the ring registers are temporaries)
    written = set()
    for ins in g.ins[start:]:
        if ins[0] not in VALU:
            continue
        for src in ins[2:5]:
            if isinstance(src, str) and src in ring:
                assert src in written, ins
        if ins[1] in ring:
            written.add(ins[1])
    assert written == ring and first_test > start
