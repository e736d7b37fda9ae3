"""launch_max_scan_u64 (ntjoin_amd/csrc/scan64_kernels.h) restated pass by pass in numpy, with faults that can be switched on, and
the inputs of its tests.  The model is no reference: the expected values of every test are np.maximum.accumulate and the restatements.
It is there to show on the CPU that an input would come out wrong if the device code had one of these faults
(tests/test_maxscan_model_cpu.py): the lookups over the running maximum are bisections, and a bisection over a partly wrong array
often lands on the right answer all the same, so an input has to be placed, and shown to discriminate.  No GPU, no library.

The passes:  1. the maximum of every tile of 1024 (k_pt_max_tile);  2. for every tile the maximum of the tiles in front of it, by one
block in rounds of 256 tiles with a carry from round to round (k_pt_max_tiles);  3. per tile the carry-in joined with the running
maximum inside the tile (k_pt_max_incl; assess.hip's k_as_cover is this pass over again and reads the maximum IN FRONT of an element).

The faults:
  tile_carry        pass 3 ignores the carry-in
  round_carry       pass 2 restarts its carry at every round of 256 tiles
  tiles_inclusive   pass 2 hands a tile its own maximum with those in front of it
  signed            every comparison as int64
  scratch_not_zero  pass 1 joins a tile's maximum with what the scratch array held before (tools/prim_check fills it with 0xCD..), as
                    code that counts on zeroed scratch would; not one of the carries: it is what the all-zero input is there for"""
import numpy as np

TILE, ROUND = 1024, 256           # elements per tile, tiles per round of pass 2
FAULTS = ("tile_carry", "round_carry", "tiles_inclusive", "signed", "scratch_not_zero")
FILL = 0xCDCDCDCDCDCDCDCD
SINGLE = (1 << 62) + 5
SIZES = [1, 2, 255, 256, 257, 1023, 1024, 1025, 4097, 262143, 262144, 262145, 524289]
PATTERNS = ("rising", "falling", "single", "records", "top_bit", "zeros")


def max_scan(a, fault=None, exclusive=False):
    """the running maximum of the uint64 array a as the three passes compute it: of a[0 .. i], or with `exclusive` of a[0 .. i) (0 in
    front of everything)"""
    assert fault is None or fault in FAULTS
    a = np.ascontiguousarray(a, dtype=np.uint64)
    n = len(a)
    n_tiles = (n + TILE - 1) // TILE
    cmp = np.int64 if fault == "signed" else np.uint64   # (every running value starts at 0: a word the comparison calls negative never wins)
    tiles = np.zeros(n_tiles * TILE, dtype=np.uint64)
    tiles[:n] = a
    tiles = tiles.view(cmp).reshape(n_tiles, TILE)
    # pass 1
    tmax = np.maximum(tiles.max(axis=1), 0)
    if fault == "scratch_not_zero":
        tmax = np.maximum(tmax, np.uint64(FILL).astype(cmp))
    # pass 2
    front = np.zeros(n_tiles, dtype=cmp)
    carry = cmp(0)
    for base in range(0, n_tiles, ROUND):
        incl = np.maximum.accumulate(tmax[base:base + ROUND])
        ex = incl if fault == "tiles_inclusive" else np.concatenate([np.zeros(1, dtype=cmp), incl[:-1]])
        if fault == "round_carry":
            carry = cmp(0)
        front[base:base + ROUND] = np.maximum(ex, carry)
        carry = max(carry, incl[-1])
    # pass 3
    if fault == "tile_carry":
        front[:] = 0
    incl = np.maximum(np.maximum.accumulate(tiles, axis=1), front[:, None])
    out = np.concatenate([front[:, None], incl[:, :-1]], axis=1) if exclusive else incl
    return out.reshape(-1)[:n].view(np.uint64).copy()


def lift_bound(arr, m, k, strict):
    """what ntjoin_amd/csrc/lift.h's lift_bound returns (there first_where of csrc/bisect.h over the same predicate), restated on its
    own: the first i in [0, m] with arr[i] >= k, or > k when strict; arr rises"""
    lo, hi = 0, m
    while lo < hi:
        mid = lo + ((hi - lo) >> 1)
        if (int(arr[mid]) > k) if strict else (int(arr[mid]) >= k):
            hi = mid
        else:
            lo = mid + 1
    return lo


def lift_range(key, rmax, r, a, b):
    "lift.h, lift_range: the candidates [lo, hi) of feature (r, a, b)"
    hi = lift_bound(key, len(key), r << 32 | b, False)
    return lift_bound(rmax, hi, r << 32 | a, True), hi


# ---- the inputs of tests/test_gpu_primitives.py::test_maxscan64 ------------------------------------------------------------------
SINGLE_PLACES = (0, 1023, 1024, 262143, 262144, "last")
# where a record of the `records` pattern begins besides the seeded places: on a tile border, one element in front of one, on tile
# borders of the second round, 44 elements in front of the second round (so the head of tile 256 lives on the round's carry: a record
# that began ON that border would need none) and on the border of the third round
RECORD_BORDERS = (1024, 2047, 3072, 262100, 300 * 1024, 400 * 1024 - 1, 524288)


def single_places(n):
    "the places of the `single` pattern at size n: above a tile all that lie below n, else the last element"
    return [p for p in SINGLE_PLACES if p == "last" or p < n] if n > TILE else ["last"]


def pattern_input(n, pattern, at=None):
    rng = np.random.default_rng(5000 + n)
    if pattern == "rising":      # the output is the input: a carry that arrives a tile early shows, and so does an exclusive maximum
        return np.arange(1, n + 1, dtype=np.uint64)
    if pattern == "falling":     # every output is a[0]: every tile and every round lives on its carry
        return np.uint64(1 << 40) - np.arange(n, dtype=np.uint64)
    if pattern == "single":      # 0 in front of `at`, the value from it on
        a = np.zeros(n, dtype=np.uint64)
        a[n - 1 if at == "last" else at] = SINGLE
        return a
    if pattern == "records":     # what the callers feed it: (record << 32) | x, the records rising
        begins = rng.random(n) < 1 / 300
        begins[[p for p in RECORD_BORDERS if p < n]] = True
        return np.cumsum(begins, dtype=np.uint64) << np.uint64(32) | rng.integers(0, 1 << 32, n, dtype=np.uint64)
    if pattern == "top_bit":     # over the whole of uint64, and in every tile words at or above 2^63
        a = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        a[rng.integers(0, TILE, (n + TILE - 1) // TILE).clip(max=n - 1 - np.arange(0, n, TILE)) + np.arange(0, n, TILE)] |= np.uint64(1 << 63)
        return a
    assert pattern == "zeros"    # the identity element as a real value
    return np.zeros(n, dtype=np.uint64)


def cases():
    "(n, pattern, at) of test_maxscan64: every pattern at every size up to 4097; the large sizes as the carries need them"
    out = []
    for n in SIZES:
        for pattern in PATTERNS:
            if n > 4097 and pattern in ("zeros", "rising", "top_bit") and not (n == 262145 and pattern != "zeros"):
                continue
            out.extend((n, pattern, at) for at in (single_places(n) if pattern == "single" else [None]))
    return out


# the faults every pattern is there for, and a size at which the model shows it: (pattern, at) -> (n, faults)
TEETH = {
    ("rising", None): (4097, ("tiles_inclusive",)),
    ("falling", None): (524289, ("tile_carry", "round_carry")),
    ("single", 0): (524289, ("tile_carry", "round_carry")),
    ("single", 1023): (4097, ("tile_carry", "tiles_inclusive")),
    ("single", 1024): (4097, ("tile_carry",)),
    ("single", 262143): (524289, ("tile_carry", "round_carry", "tiles_inclusive")),
    ("single", 262144): (524289, ("tile_carry",)),
    ("single", "last"): (262143, ("tiles_inclusive",)),
    ("records", None): (524289, ("tile_carry", "round_carry", "tiles_inclusive")),
    ("top_bit", None): (4097, ("signed", "tile_carry")),
    ("zeros", None): (4097, ("scratch_not_zero",)),
}
