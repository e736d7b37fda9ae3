"""GPU tests of the sketch stage over the range of (k, w) the library accepts (mxg_create: 1 <= k <= 1024, 1 <= w <= 2^24), always
bit for bit against the CPU oracle:
  * k from 1 to 1024 on every hash route (dense; k_hash_sparse + k_reorder_w; k_reorder; the one-thread-per-entry path; the stretch
    kernels behind few candidates, on the device and through the host) -- the k at which srol_var's zero branches are reached
    (k - 4 or k a multiple of 33 or 31), group and tail shapes of the position tables, byte and 16-base borders, the extremes;
  * k_gap_fix with the longest stretches it accepts at k = 1009, 1023, 1024, at every alignment of the stretch's first base;
  * w on both sides of every threshold at which the driver changes route (768, 2048, 4096, 4224) and far beyond them;
  * split loads, a FASTA file through the device parser and the accepted / refused edges of mxg_create at the extremes.
The oracle's sketches are computed once per (records, k, w, variant) and shared by the tests of this file."""
import os
import random
import re

import numpy as np
import pytest

from tests import _oracle

pytestmark = pytest.mark.gpu

KNOBS = ("MXG_REORDER_W", "MXG_WAVE_CAP", "MXG_SPARSE_S", "MXG_DEV_GAPS", "MXG_BS", "MXG_BS_SELECT", "MXG_SPARSE_BATCH_KMERS",
         "MXG_DENSE_BATCH_KMERS", "MXG_GAP_WHOLE", "MXG_STRETCH_DENSE", "MXG_SEL_INLINE", "MXG_DEV_CAND", "MXG_GAP_DEV_CAP",
         "MXG_HOST_INGEST", "MXG_HOST_TSV")
EINVAL = -1


@pytest.fixture
def env():
    "none of the route knobs set; whatever the test sets is taken back and the caller's values return"
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    yield os.environ
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def _rnd(rng, n):
    return "".join(rng.choices("ACGT", k=n))


_WANT = {}


def _want(oracle, key, recs, k, w, variant):
    "the oracle's (out_hash, pos, forward) of every record, computed once per key"
    key = (key, k, w, variant)
    if key not in _WANT:
        v = _oracle.V1_MIN if variant == "v1" else _oracle.V2_SUM
        _WANT[key] = [[(h, p, f) for h, p, f, _ in oracle.sketch(seq, k, w, v)] for _, seq in recs]
    return _WANT[key]


def _check(oracle, key, recs, k, w, variant="v2", **kw):
    from ntjoin_amd.engine import MxEngine
    want = _want(oracle, key, recs, k, w, variant)
    with MxEngine(k=k, w=w, variant=variant, **kw) as eng:
        eng.add_records("x", 1.0, recs)
        eng.sketch()
        sk = eng.get_sketch(0)
        st = eng.stats()
        st["knobs"] = eng.knobs()
    first = sk["record_first"]
    assert len(first) == len(recs) + 1
    for r, (rid, _) in enumerate(recs):
        lo, hi = int(first[r]), int(first[r + 1])
        got = list(zip(sk["out_hash"][lo:hi].tolist(), sk["pos"][lo:hi].tolist(), sk["forward"][lo:hi].tolist()))
        assert got == want[r], (rid, k, w, variant, kw, len(got), len(want[r]))
    return st


# -----------------------------------------------------------------------------------------------------------------
# 1. k over the accepted range on every hash route
# -----------------------------------------------------------------------------------------------------------------
K_LIST = (1, 2, 3, 4, 5, 35, 36, 37, 66, 70, 97, 103, 127, 128, 129, 199, 200, 201, 255, 256, 257, 511, 512, 513, 995, 996, 997,
          1008, 1009, 1023, 1024)
_K_RECS = {}


def _k_records(k, w):
    if (k, w) in _K_RECS:
        return _K_RECS[(k, w)]
    rng = random.Random(1000 * w + k)
    runs = w + 20   # runs of valid bases in the records with an N at a fixed period: enough k-mers for windows where a run holds any
    recs = [("random", _rnd(rng, 20000))]
    recs += [(f"len{n}", _rnd(rng, n)) for n in (k - 1, k, k + 1, k + w - 2, k + w - 1, k + w)]
    recs += [("n_every_k-1", "".join(_rnd(rng, k - 1) + "N" for _ in range(runs))),      # no k-mer at all
             ("n_every_k", "".join(_rnd(rng, k) + "N" for _ in range(runs))),            # one k-mer per run
             ("n_every_k+1", "".join(_rnd(rng, k + 1) + "N" for _ in range(runs))),      # two
             ("lower", _rnd(rng, max(3000, 2 * k + 2 * w)).lower()),
             ("polyA", _rnd(rng, 1500 + k) + "A" * 6000 + _rnd(rng, 1500 + k)),
             ("unit7", _rnd(rng, 1500 + k) + "ACGGTCA" * 900 + _rnd(rng, 1500 + k))]
    _K_RECS[(k, w)] = recs
    return recs


def _k_sweep(oracle, w, variant, after=None, **kw):
    "every k of K_LIST through the route the caller has set up -> {k: stats}"
    stats = {}
    for k in K_LIST:
        recs = _k_records(k, w)
        want = _want(oracle, "k_sweep", recs, k, w, variant)
        if k >= 4:  # (k <= 3: at most 64 distinct k-mers; the windows are still compared)
            assert any(want), (k, w)
        assert want[7] == [] and want[1] == [] and want[4] == []   # no k-mer / k - 1 bases / w - 1 k-mers: no minimizer
        assert len(want[6]) >= 1 and len(want[5]) >= 1 or k < 4     # exactly w and w + 1 k-mers: a window
        stats[k] = _check(oracle, "k_sweep", recs, k, w, variant, **kw)
        if after:
            after(k, stats[k])
    assert sorted(stats) == sorted(K_LIST)
    return stats


VARIANTS = pytest.mark.parametrize("variant", ["v2", "v1"])


@VARIANTS
def test_k_range_dense_route(oracle, env, variant):
    "dense_only: k_hash_dense warms up with k steps through fetch16 for every strip; w = 10"
    def after(k, st):
        assert st["dense_kmers"] > 0 and st["candidates"] == 0 and st["select_slices"] == 0, (k, st)
    _k_sweep(oracle, 10, variant, after, dense_only=True)


# The sparse routes at w = 100 need few enough candidates per window: the library's own 18 would be 0.18 of the k-mers, above the
# 1/8 at which it takes the dense route.  Six, as test_exact_hash_from_position_tables_every_group_shape has them.
SPARSE = {"cand_per_window": 6}


def _sparse_ran(k, st, c=6):
    # the candidates are the sparse kernel's; k = 32 is not in the list, so neither the bit-sliced filter nor the slice kernel ran.
    # (k <= 3 has at most 32 distinct canonical k-mers: with probability (1 - c/100)^32 = 0.14 at c = 6 none of them is below the
    # threshold, and the whole input is one candidate-free stretch.  136 at k = 4: 2e-4 at c = 6 but 0.06 at c = 2; 512 at k = 5.)
    assert st["bs_filter_bases"] == 0 and st["select_slices"] == 0, (k, st)
    assert st["candidates"] > 0 or k < (4 if c >= 6 else 5), (k, st)


@VARIANTS
def test_k_range_default_sparse_route(oracle, env, variant):
    "k_hash_sparse (init_direct per strip: rotation by k - 4) and k_reorder_w (init_pos: groups of 32 bases, rotations of 32 j)"
    _k_sweep(oracle, 100, variant, _sparse_ran, **SPARSE)


@VARIANTS
def test_k_range_block_per_slice_reorder(oracle, env, variant):
    "MXG_REORDER_W=0: k_reorder, init_direct for every candidate (no statistic tells it from k_reorder_w: the knob report does)"
    env["MXG_REORDER_W"] = "0"

    def after(k, st):
        _sparse_ran(k, st)
        assert "MXG_REORDER_W=0" in st["knobs"]
    _k_sweep(oracle, 100, variant, after, **SPARSE)


@VARIANTS
def test_k_range_one_thread_per_entry(oracle, env, variant):
    "MXG_WAVE_CAP=9000, MXG_SPARSE_S=256: arena slices beyond k_reorder's LDS queue (no statistic of its own: the knob report)"
    env["MXG_WAVE_CAP"] = "9000"
    env["MXG_SPARSE_S"] = "256"

    def after(k, st):
        _sparse_ran(k, st)
        assert "MXG_WAVE_CAP=9000" in st["knobs"] and "MXG_SPARSE_S=256" in st["knobs"]
    _k_sweep(oracle, 100, variant, after, **SPARSE)


def _repeat_kmer_is_candidate(oracle, k, w, c, variant):
    """is the homopolymer's k-mer or one of the seven of the 7-base unit below the candidate threshold (sparse_plan: the top 32 bits
    of the canonical hash against c / w of 2^32, made even)?  Then the repeat is no candidate-free stretch but a flood of candidates."""
    tau = int(c / w * 4294967296.0) & ~1
    v = _oracle.V1_MIN if variant == "v1" else _oracle.V2_SUM
    for seq in ("A" * k, ("ACGGTCA" * (k // 7 + 2))[:k + 6]):
        mh, _, _, ok = oracle.kmer_hashes(seq, k, v)
        if any((int(x) >> 32) < tau for x in mh):
            return True
    return False


@VARIANTS
def test_k_range_stretches_on_the_device(oracle, env, variant):
    """two candidates per window and MXG_DEV_GAPS=1: candidate-free stretches everywhere -- k_gap_fix (warm_up from its LDS copy of
    the stretch's bases, k - 1 bases beyond the last k-mer), k_stretch_tiles for the homopolymer's stretch of 6000 - k + 1 > 4096
    k-mers.  Every batch ends the common way, with two exceptions the code accounts for.  (i) k <= 3 may leave no candidate at all:
    BatchReport::ended_well leaves a batch without candidates to the host (finish_from_scratch), which counts nothing.  (ii) Where
    the homopolymer's k-mer or one of the unit's seven is itself a candidate, the repeat holds a candidate every one or seven k-mers
    where the arena slices were sized for two per hundred: the hash kernel reports CW_ARENA_NEED and the one batch is redone
    with the room it asked for (measured with MXG_DEBUG_BATCH=1: `ovf 577` ... `ovf 4096` in exactly the ten (k, variant) pairs
    for which the oracle's hashes say so: v2 255, 511; v1 5, 66, 103, 128, 129, 201, 996, 997)."""
    env["MXG_DEV_GAPS"] = "1"
    floods = []

    def after(k, st):
        _sparse_ran(k, st, 2)
        assert st["dense_kmers"] > 0 and "MXG_DEV_GAPS=1" in st["knobs"], (k, st)
        if _repeat_kmer_is_candidate(oracle, k, 100, 2, variant):
            floods.append(k)
        elif st["candidates"]:
            assert st["deferred_stretches"] > 0, (k, st)          # the homopolymer: to the tile kernel
            assert st["batches_redone"] == 0 and st["sync_assemblies"] == 0 and st["retried_assemblies"] == 0, (k, st)
    _k_sweep(oracle, 100, variant, after, cand_per_window=2)
    assert len(floods) < len(K_LIST) // 2, floods   # (eight k-mers at 2 %, either strand for v1: the route is witnessed at most k)


@VARIANTS
def test_k_range_stretches_through_the_host(oracle, env, variant):
    "two candidates per window and MXG_DEV_GAPS=0: the host finds the stretches and the tile kernel sketches them"
    env["MXG_DEV_GAPS"] = "0"

    def after(k, st):
        _sparse_ran(k, st, 2)
        assert st["dense_kmers"] > 0 and st["deferred_stretches"] == 0, (k, st)
    _k_sweep(oracle, 100, variant, after, cand_per_window=2)


# -----------------------------------------------------------------------------------------------------------------
# 2. k_gap_fix: the longest stretches it accepts, at large k, at every alignment of the stretch's first base
# -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1009, 1023, 1024])
def test_gap_fix_longest_stretch_at_large_k(oracle, env, k):
    """k_gap_fix keeps a stretch's bases in 324 words of LDS and accepts n <= 4096 k-mers that span <= 4096 + 1024 bases: at
    k = 1024 a stretch of 4096 k-mers whose first base is at offset 15 of its word loads 322 of them.  One record per sketch:
    flank, "A" * L, flank; the candidate-free stretch is the homopolymer's L - k + 1 k-mers and what the flanks add up to their
    nearest candidates -- the same in every record, since a record differs from the next only in L and in how many bases of
    the first flank's START it keeps.  L - k + 1 runs from 4096 - 60 to 4096 + 4 with the alignment cycling; then both sides
    of the length at which the stretch stops fitting, at all sixteen alignments."""
    env["MXG_DEV_GAPS"] = "1"
    w = 200
    rng = random.Random(k)
    head, tail = _rnd(rng, 2500 + 15), _rnd(rng, 2500)

    def run(L, cut):
        rec = [("r", head[cut:] + "A" * L + tail)]
        st = _check(oracle, ("gap_fix", L, cut), rec, k, w, "v2", cand_per_window=16)
        assert st["batches_redone"] == 0 and st["sync_assemblies"] == 0, (L, cut, st)
        return st["deferred_stretches"]

    lens = list(range(4096 - 60 + k - 1, 4096 + 4 + k))
    deferred = [run(L, i % 16) for i, L in enumerate(lens)]
    print(f"k={k}: deferred_stretches over L - k + 1 = 4036..4100: {deferred}")
    assert deferred[0] == 0 and deferred[-1] > 0
    first = next(i for i, d in enumerate(deferred) if d)
    assert all(d == 0 for d in deferred[:first]) and all(d > 0 for d in deferred[first:])
    for cut in range(16):  # the four longest stretches that stay, the shortest that leaves
        for i in range(first - 4, first):
            assert run(lens[i], cut) == 0, (i, cut)
        assert run(lens[first], cut) > 0, cut


# -----------------------------------------------------------------------------------------------------------------
# 3. w on both sides of every threshold
# -----------------------------------------------------------------------------------------------------------------
W_LIST = (768, 769, 2048, 2049, 2500, 4096, 4097, 4224, 4225, 5000, 10000, 65535, 65536, 100000)
_W_RECS = {}


def _w_records(k, w):
    if (k, w) in _W_RECS:
        return _W_RECS[(k, w)]
    rng = random.Random(7 * w + k)
    recs = [("random", _rnd(rng, 2 * w + w // 2 + k)),
            ("one_window", _rnd(rng, w + k - 1)),          # exactly w k-mers: one minimizer
            ("no_window", _rnd(rng, w + k - 2)),           # w - 1 k-mers: none
            ("polyA", "A" * (2 * w)),                      # every window ties
            ("unit7", ("ACGGTCA" * (2 * w // 7 + 1))[:2 * w]),
            ("with_n", _rnd(rng, 3 * w // 2) + "N" * 5 + _rnd(rng, 3 * w // 2 - 5))]
    assert max(len(s) for _, s in recs) <= 300_000
    _W_RECS[(k, w)] = recs
    return recs


def _w_check(oracle, k, w, n_free=False, **kw):
    recs = _w_records(k, w)
    want = _want(oracle, "w_sweep", recs, k, w, "v2")
    assert len(want[1]) == 1 and want[2] == [] and len(want[0]) >= 2 and len(want[3]) == 2 * w - k + 1 - w + 1
    if n_free:  # (a contig of several runs makes the slice kernel's halo longer than ceil(w / S): see bs_select_halo)
        return _check(oracle, "w_sweep_n_free", recs[:5], k, w, **kw)
    return _check(oracle, "w_sweep", recs, k, w, **kw)


@pytest.mark.parametrize("w", W_LIST)
def test_w_thresholds_k32_routes(oracle, env, w):
    """k = 32: the bit-sliced filter with the slice kernel (default), with the batch kernels (MXG_BS_SELECT=0), the rolling-hash
    kernel (MXG_BS=0), the dense route.  The slice kernel takes halos of up to 12 strips: at the strip length 352 of w > 768
    that is w <= 4224."""
    st = _w_check(oracle, 32, w)
    assert st["bs_filter_bases"] > 0 and st["candidates"] > 0, st
    if w > 4224:
        assert st["select_slices"] == 0, st       # ceil(w / 352) > 12: the route refuses
    free = _w_check(oracle, 32, w, n_free=True)
    assert (free["select_slices"] > 0) == (w <= 4224), (w, free)
    env["MXG_BS_SELECT"] = "0"
    st = _w_check(oracle, 32, w)
    assert st["bs_filter_bases"] > 0 and st["select_slices"] == 0 and st["candidates"] > 0, st
    env.pop("MXG_BS_SELECT")
    env["MXG_BS"] = "0"
    st = _w_check(oracle, 32, w)
    assert st["bs_filter_bases"] == 0 and st["select_slices"] == 0 and st["candidates"] > 0, st
    env.pop("MXG_BS")
    st = _w_check(oracle, 32, w, dense_only=True)
    assert st["dense_kmers"] > 0 and st["candidates"] == 0 and st["bs_filter_bases"] == 0, st


@pytest.mark.parametrize("w,ran", [(768, True), (769, False)])
def test_w_select_halo_of_twelve_and_thirteen_strips(oracle, env, w, ran):
    "MXG_SPARSE_S=64: ceil(w / 64) = 12 strips of halo at w = 768, which the slice kernel takes, and 13 at w = 769, which it refuses"
    env["MXG_SPARSE_S"] = "64"
    st = _w_check(oracle, 32, w, n_free=True)
    assert (st["select_slices"] > 0) == ran and st["bs_filter_bases"] > 0 and "MXG_SPARSE_S=64" in st["knobs"], st
    st = _w_check(oracle, 32, w)
    assert st["bs_filter_bases"] > 0, st
    if not ran:
        assert st["select_slices"] == 0, st


@pytest.mark.parametrize("w", W_LIST)
def test_w_thresholds_general_sparse_route(oracle, env, w):
    """k = 33: the general sparse route; with two candidates per window its candidate-free stretches are sketched by k_gap_fix and the
    tile kernel up to w = 2048 and by the dense pipeline (process_gaps) beyond, whoever found them -- MXG_DEV_GAPS=1 is not taken
    above w = 2048 (the handle has read the knob; no stretch is placed or deferred on the device)"""
    st = _w_check(oracle, 33, w)
    assert st["candidates"] > 0 and st["bs_filter_bases"] == 0 and st["select_slices"] == 0, st
    env["MXG_DEV_GAPS"] = "1"
    st = _w_check(oracle, 33, w, cand_per_window=2)
    assert "MXG_DEV_GAPS=1" in st["knobs"] and st["candidates"] > 0 and st["dense_kmers"] > 0, st
    if w > 2048:
        assert st["deferred_stretches"] == 0, st   # nothing went through the device route
    else:
        assert st["batches_redone"] == 0 and st["sync_assemblies"] == 0, st
    env["MXG_DEV_GAPS"] = "0"
    st = _w_check(oracle, 33, w, cand_per_window=2)
    assert st["candidates"] > 0 and st["dense_kmers"] > 0 and st["deferred_stretches"] == 0, st


def test_accepted_and_refused_extremes(oracle, env):
    "k = 1024 with w = 2^24 is accepted and a 1 kbp record has no minimizer; one step beyond either end is MXG_EINVAL"
    from ntjoin_amd.engine import MxEngine, MxError
    rng = random.Random(3)
    recs = [("kbp", _rnd(rng, 1000)), ("two_kmers", _rnd(rng, 1025))]
    with MxEngine(k=1024, w=1 << 24) as eng:
        eng.add_records("x", 1.0, recs)
        eng.sketch()
        sk = eng.get_sketch(0)
        assert len(sk["out_hash"]) == 0 and sk["record_first"].tolist() == [0, 0, 0]
    _check(oracle, "extreme", recs, 1, 1 << 24)
    for k, w in ((0, 100), (1025, 100), (32, 0), (32, (1 << 24) + 1)):
        with pytest.raises(MxError) as err:
            MxEngine(k=k, w=w)
        assert err.value.code == EINVAL, (k, w, err.value.code)


# -----------------------------------------------------------------------------------------------------------------
# 4. split loads and the FASTA route at the extremes
# -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,w", [(1024, 50), (32, 5000)])
def test_split_shards_at_large_k_and_w(oracle, tmp_path, env, k, w):
    "the split planner's halo is k + w - 1: shards of a file concatenate to the whole, and the whole is the oracle's"
    from tests.test_gpu_split import _genome, _pieces, _whole
    fa = str(tmp_path / "g.fa")
    _genome(fa, 5 + k, [30_000, 500, 120_000, 31, 1_000, 60_000, 40, 45_000])
    whole = _whole(fa, k, w)
    want = [(r, h, p) for r, (_, seq) in enumerate(_oracle.read_fasta(fa)) for h, p, _, _ in oracle.sketch(seq, k, w)]
    assert len(want) > (1000 if w == 50 else 50)
    assert list(zip(whole["record"].tolist(), whole["out_hash"].tolist(), whole["pos"].tolist())) == want
    for n_shards in (3, 7):
        got, _, _, _ = _pieces(fa, k, w, n_shards)
        for key in whole:
            assert np.array_equal(whole[key], got[key]), (n_shards, key)


def test_fasta_through_the_device_parser_at_k_1024(oracle, tmp_path, env):
    "CRLF and ragged lines, an N run, a lower-case record; the TSV with the k-mer column (the host writer above k = 200)"
    from ntjoin_amd.engine import MxEngine
    rng = random.Random(1024)
    recs = [("plain", _rnd(rng, 9000)), ("with_n some words", _rnd(rng, 4000) + "N" * 300 + _rnd(rng, 3500)), ("lower", _rnd(rng, 5000).lower()),
            ("short", _rnd(rng, 1023)), ("ragged", _rnd(rng, 6000))]
    fa = str(tmp_path / "k.fa")
    with open(fa, "w", newline="") as fh:
        for i, (rid, s) in enumerate(recs):
            eol = "\r\n" if i % 2 == 0 else "\n"
            fh.write(">" + rid + eol)
            at = 0
            while at < len(s):
                n = 70 if rid != "ragged" else rng.choice([1, 7, 60, 61, 200])
                fh.write(s[at:at + n] + eol)
                at += n
    want = str(tmp_path / "want.tsv")
    oracle.fasta_to_tsv(fa, want, 1024, 10)
    with open(want, "rb") as fh:
        want = fh.read()
    assert re.search(rb":[acgt]{1024}[ \n]", want) and re.search(rb":[ACGT]{1024}[ \n]", want) and b"short\t\n" in want
    out = str(tmp_path / "got.tsv")
    with MxEngine(k=1024, w=10, threads=3) as eng:
        eng.add_fasta("x", 1.0, fa)
        eng.sketch()
        eng.write_tsv(0, out, with_pos=True, with_strand=False, with_seq=True)
        assert eng.stats()["minimizers"] > 1000
    with open(out, "rb") as fh:
        got = fh.read()
    assert got == want
