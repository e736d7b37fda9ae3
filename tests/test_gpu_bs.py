"""GPU tests of the k = 32 route of the sketch stage (csrc/bs_kernels.h, sketch_bs.hip: k_bs_select; k_bs_count / k_bs_reorder_w):

  * the generated filter kernel against the direct ring formula on random bases (standalone binary built with the library:
    layout kernel + filter over whole chunks, ragged tail, first / middle / last chunks compared word for word);
  * the three routes of the library -- bit-sliced filter + the slice kernel k_bs_select (default), bit-sliced filter + the batch
    kernels count -> reorder -> resolve (MXG_BS_SELECT=0), the rolling-hash kernel (MXG_BS=0) -- against the CPU oracle on the
    same records, bit for bit, with the statistics saying which route ran;
  * slices that outgrow their LDS queue (MXG_SEL_QCAP) work in global memory, and a batch without a region left is redone;
  * inputs the filter does not take (k != 32, the min(fwd, rev) variant) still go the old way;
  * the k_emit that a single-batch assembly holds back for the next assembly's slice kernel (MXG_DEFER_EMIT, MXG_STAGGER): the same
    sketches as with every emit in its own place;
  * the request array of k_sel_stretch at its capacity (MXG_SEL_IREQ_CAP; csrc/sel_requests.h): every capacity from one request to
    one more than a small input makes, batches that walk what earlier batches and other assemblies left in the array, realistic
    records at a handful of capacities, the fused call -- no stale request is taken, no minimizer comes out twice.
"""
import os
import random
import subprocess

import pytest

from tests import _oracle
from tests.test_gpu_scale_paths import _check, _records

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_KNOBS = ("MXG_GAP_POOL", "MXG_BS", "MXG_BS_SELECT", "MXG_SEL_QCAP", "MXG_SEL_RK", "MXG_GAP_WHOLE", "MXG_GAP_DEV_CAP", "MXG_SPARSE_BATCH_KMERS", "MXG_WAVE_CAP", "MXG_SPARSE_S", "MXG_DEV_GAPS", "MXG_SEL_INLINE",
               "MXG_SEL_IREQ_CAP", "MXG_DEFER_EMIT", "MXG_STAGGER")


@pytest.fixture
def env():
    saved = {k: os.environ.get(k) for k in ROUTE_KNOBS}
    yield os.environ
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


@pytest.mark.parametrize("mbp,tt", [(1, 164), (3, 40), (2, 0), (1, 16383)])
def test_filter_kernel_against_direct_formula(mbp, tt):
    exe = os.path.join(REPO, "ntjoin_amd", "bin", "bs_check")
    assert os.path.exists(exe), "ntjoin_amd/bin/bs_check missing: run __graft_entry__.build()"
    r = subprocess.run([exe, str(mbp), str(tt)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "verify: ok" in r.stdout


def _bases(recs):
    return sum(len(s) for _, s in recs)


@pytest.mark.parametrize("seed,w", [(11, 200), (12, 1000), (13, 150)])
def test_three_routes_agree_with_the_oracle(oracle, env, seed, w):
    recs = _records(seed)
    env["MXG_BS"] = "1"
    st = _check(oracle, recs, 32, w)
    assert st["bs_filter_bases"] == _bases(recs), "the k = 32 route did not run"
    assert st["candidates"] > 0
    env["MXG_BS_SELECT"] = "0"
    st = _check(oracle, recs, 32, w)
    assert st["bs_filter_bases"] == _bases(recs)
    env["MXG_BS_SELECT"] = "1"
    env["MXG_BS"] = "0"
    st = _check(oracle, recs, 32, w)
    assert st["bs_filter_bases"] == 0


@pytest.mark.parametrize("S,w", [(320, 1000), (64, 200), (128, 500), (512, 1000), (1024, 777)])
def test_select_route_runs_and_agrees(oracle, env, S, w):
    """k_bs_select on records with N runs, low-complexity islands and short records, strips of every template size"""
    env["MXG_SPARSE_S"] = str(S)
    env["MXG_BS"] = "1"
    env["MXG_BS_SELECT"] = "1"
    st = _check(oracle, _records(100 + S), 32, w)
    assert st["select_slices"] > 0, "k_bs_select did not run"
    env["MXG_DEV_GAPS"] = "1"      # candidate-free stretches stay on the device: few candidates per window make many
    st = _check(oracle, _records(200 + S), 32, w, cand_per_window=3)
    assert st["select_slices"] > 0
    env["MXG_SPARSE_BATCH_KMERS"] = "50000"
    st = _check(oracle, _records(300 + S), 32, w, cand_per_window=5)
    assert st["select_slices"] > 0


@pytest.mark.parametrize("w", [1000, 2500, 200])
def test_select_route_is_the_default_for_small_inputs(oracle, env, w):
    """no strip-length knob: an input of a few hundred kbp takes the same route as a genome (strips long enough for the
    slice kernel's halo at any w it covers)"""
    env.pop("MXG_SPARSE_S", None)
    st = _check(oracle, _records(400 + w), 32, w)
    assert st["select_slices"] > 0


def test_select_slices_beyond_their_queue(oracle, env):
    """MXG_SEL_QCAP=64: nearly every slice has more raw candidates than its LDS queue holds and works in a region of global
    memory; the results do not change"""
    env["MXG_SPARSE_S"] = "320"
    env["MXG_SEL_QCAP"] = "64"
    env["MXG_DEV_GAPS"] = "1"
    st = _check(oracle, _records(51), 32, 1000)
    assert st["select_slices"] > 0
    st = _check(oracle, _records(52), 32, 300, cand_per_window=12)
    assert st["select_slices"] > 0


@pytest.mark.parametrize("dev_gaps", ["0", "1"])
def test_select_slice_that_gives_up_is_redone(oracle, env, dev_gaps):
    """MXG_SEL_RK=4: a slice has room for four selected candidates, so nearly every slice gives up (its output would be
    truncated); the kernel's flag sends the batch through the other route, with and without the device's stretch route"""
    env["MXG_SPARSE_S"] = "320"
    env["MXG_SEL_RK"] = "4"
    env["MXG_DEV_GAPS"] = dev_gaps
    _check(oracle, _records(61), 32, 1000)
    _check(oracle, _records(62), 32, 300, cand_per_window=12)


def test_select_stretch_ends_behind_the_slice(oracle, env):
    """candidate-free stretches far longer than a slice's halo (a satellite-like array, a homopolymer, a contig without any
    candidate): the reporting slice walks on to the stretch's end"""
    rng = random.Random(5)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    unit = rnd(171)
    recs = [("sat", rnd(30000) + unit * 400 + rnd(30000)), ("polyA", rnd(5000) + "A" * 90000 + rnd(2000)),
            ("unit7", ("ACGGTCA" * 20000)[:100000]), ("plain", rnd(200000)), ("polyT_end", rnd(3000) + "T" * 50000)]
    env["MXG_SPARSE_S"] = "320"
    env["MXG_DEV_GAPS"] = "1"
    for c in (2, 10):
        st = _check(oracle, recs, 32, 1000, cand_per_window=c)
        assert st["select_slices"] > 0


@pytest.mark.parametrize("dev_gaps", ["0", "1"])
def test_stretches_are_sketched_behind_the_slice_kernel(oracle, env, dev_gaps):
    """few candidates per window on plain random sequence: hundreds of candidate-free stretches just over a window long, between two
    candidates of a slice, at a contig's start and end, reaching past the slice's strips -- k_sel_stretch sketches them one wave per
    slice and puts their minimizers into the slice's row (several stretches in one slice: the last one first); with a window of
    2500 and 3 candidates a stretch is taken in pieces; MXG_SEL_INLINE=0: the same sketch with every stretch through k_gap_fix"""
    rng = random.Random(77)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    recs = [("a", rnd(700000)), ("b", rnd(1500)), ("c", rnd(1031)), ("d", rnd(300000)), ("n_inside", rnd(40000) + "N" + rnd(50000) + "NNNN" + rnd(800)),
            ("e", rnd(2200)), ("f", rnd(450000))]
    env["MXG_SPARSE_S"] = "320"
    env["MXG_DEV_GAPS"] = dev_gaps
    for w, c in ((1000, 4), (1000, 7), (300, 3), (2500, 3), (64, 2)):
        st = _check(oracle, recs, 32, w, cand_per_window=c)
        assert st["select_slices"] > 0 and st["deferred_stretches"] == 0, (w, c)
        assert st["slice_stretches"] > 5, (w, c, st["slice_stretches"])
    env["MXG_SEL_INLINE"] = "0"
    st = _check(oracle, recs, 32, 1000, cand_per_window=4)
    assert st["slice_stretches"] == 0


def test_low_complexity_stretches_stay_on_the_device(oracle, env):
    """di- and trinucleotide runs longer than a window: every second / third k-mer of the run is a minimizer (the rightmost of
    equal hashes wins each time the window moves on) -- hundreds per candidate-free stretch, all of them through k_gap_fix"""
    rng = random.Random(8)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    recs = [("di", rnd(20000) + "AC" * 900 + rnd(7000) + "AT" * 1400 + rnd(9000)),
            ("tri", rnd(3000) + "GGC" * 800 + rnd(30000) + "GGC" * 1000 + rnd(100)),
            ("plain", rnd(150000)), ("di_end", rnd(9000) + "TG" * 1200),
            # invalid bases inside the stretch: its k-mers come from two or three valid runs
            ("di_n", rnd(12000) + "AC" * 500 + "N" + "AC" * 600 + rnd(8000) + "AT" * 450 + "N" * 20 + "AT" * 450 + "N" * 300 + "AT" * 300
             + rnd(5000)),
            ("tri_n", rnd(700) + "N" * 5 + "GGC" * 700 + "NN" + rnd(40000))]
    env["MXG_DEV_GAPS"] = "1"
    for w in (1000, 600):
        st = _check(oracle, recs, 32, w)
        assert st["select_slices"] > 0
        assert st["deferred_stretches"] == 0, st["deferred_stretches"]
    # a pool of 300 entries: the stretches that find it used up go to the host and through the tile kernel, same sketch
    env["MXG_GAP_POOL"] = "300"
    st = _check(oracle, recs, 32, 1000)
    assert st["deferred_stretches"] > 0
    env.pop("MXG_GAP_POOL")
    # more invalid bases inside a stretch than the block's words take: handed over as well
    recs2 = [("wide_n", rnd(6000) + "AT" * 900 + "N" * 3000 + "AT" * 900 + rnd(9000)), ("plain", rnd(90000))]
    st = _check(oracle, recs2, 32, 1000)
    assert st["deferred_stretches"] > 0


def test_long_stretches_are_reported_in_pieces(oracle, env):
    """candidate-free stretches longer than k_gap_fix's 4096 k-mers (a homopolymer of 90 kb, a satellite-like array, dinucleotide
    runs, one of them across N): the slice kernel reports them in pieces that overlap by one window, every piece after the first
    leaving out the arg-min of the window it shares with the piece before it -- nothing goes to the host.  Then with a stretch
    pool of 300 entries: pieces that find the pool used up are handed over, marked pieces among them (the tile kernel starts those
    at their second window), same sketch."""
    rng = random.Random(23)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    unit = rnd(171)
    recs = [("polyA", rnd(5000) + "A" * 90000 + rnd(2000)), ("sat", rnd(30000) + unit * 300 + rnd(30000)),
            ("di", rnd(800) + "AC" * 9000 + rnd(7000) + "TG" * 2300 + "N" * 3 + "TG" * 2500 + rnd(900)),
            ("unit7_whole", ("ACGGTCA" * 6000)[:40000]), ("plain", rnd(120000)), ("polyT_end", rnd(3000) + "T" * 20000)]
    env["MXG_SPARSE_S"] = "320"
    env["MXG_DEV_GAPS"] = "1"
    for w, c in ((1000, 10), (2048, 10), (300, 4), (1000, 2)):
        st = _check(oracle, recs, 32, w, cand_per_window=c)
        assert st["select_slices"] > 0 and st["deferred_stretches"] == 0, (w, c, st["deferred_stretches"])
    env["MXG_GAP_POOL"] = "300"
    st = _check(oracle, recs, 32, 1000, cand_per_window=10)
    assert st["deferred_stretches"] > 3
    env.pop("MXG_GAP_POOL")
    env["MXG_GAP_WHOLE"] = "1"      # the long ones whole, to the host: rounds 3 and 4
    st = _check(oracle, recs, 32, 1000, cand_per_window=10)
    assert st["deferred_stretches"] > 3
    env.pop("MXG_GAP_WHOLE")
    env["MXG_GAP_DEV_CAP"] = "64"   # more stretches than the arrays hold: the batch is enqueued again, then redone
    _check(oracle, recs + [(f"x{i}", rnd(9000)) for i in range(40)], 32, 1000, cand_per_window=2)


def test_stretch_counts_around_the_rank_kernels_last_block(oracle, env):
    """k_gap_post ranks sixteen stretches per block: with per-stretch arrays (and placing blocks) for a number of stretches that is
    no multiple of sixteen, a batch whose stretch count falls into the last, partial block must still have every stretch ranked
    (the grid rounded down until round 6: those stretches' minimizers landed at stale offsets).  A sweep of record lengths
    walks the count through 50 ... 90 stretches against arrays for 72: counts beyond 72 are enqueued again / redone, all others
    are placed on the device."""
    env["MXG_DEV_GAPS"] = "1"
    env["MXG_GAP_DEV_CAP"] = "72"
    rng = random.Random(66)
    placed = 0
    for L in range(60000, 124000, 2000):
        rec = [("r%d" % L, "".join(rng.choice("ACGT") for _ in range(L)))]
        st = _check(oracle, rec, 32, 200, cand_per_window=3)
        assert st["select_slices"] > 0
        placed += 1 if st["batches_redone"] == 0 and st["retried_assemblies"] == 0 else 0
    assert placed >= 4, placed      # (the sweep did reach counts the device route keeps)


def test_many_batches_and_overflow_on_the_bs_route(oracle, env):
    env["MXG_SPARSE_BATCH_KMERS"] = "30000"
    st = _check(oracle, _records(21), 32, 200)
    assert st["bs_filter_bases"] > 0 or os.environ.get("MXG_BS") == "0"  # (MXG_BS=0: the rolling-hash route is under test)
    env["MXG_WAVE_CAP"] = "8"       # every slice outgrows its queue: the batch is redone with the capacity it asked for
    env["MXG_SPARSE_S"] = "128"
    st = _check(oracle, _records(22), 32, 200)
    assert st["bs_filter_bases"] > 0 or os.environ.get("MXG_BS") == "0"  # (MXG_BS=0: the rolling-hash route is under test)
    env["MXG_WAVE_CAP"] = "9000"    # queues beyond LDS: such a batch takes the rolling-hash kernel instead
    env["MXG_SPARSE_S"] = "256"
    _check(oracle, _records(23), 32, 200)


def test_inputs_the_filter_does_not_take(oracle, env):
    st = _check(oracle, _records(31), 31, 200)
    assert st["bs_filter_bases"] == 0
    st = _check(oracle, _records(32), 32, 300, cand_per_window=4, variant="v1")
    assert st["bs_filter_bases"] == 0


def test_run_borders_and_short_records(oracle, env):
    """N runs every few hundred bases, records shorter than a window, records of exactly k .. k + w bases: positions whose
    32-mer crosses a run border are set in the bitmap (the filter sees bases, not runs) and must be masked by the batch kernels"""
    rng = random.Random(77)
    recs = []
    for r in range(60):
        n = rng.choice([31, 32, 33, 100, 231, 232, 233, 700, 3000, 9000])
        s = [rng.choice("ACGT") for _ in range(n)]
        for _ in range(n // 400):
            p = rng.randrange(0, n)
            s[p:p + rng.choice([1, 2, 31, 32, 33, 90])] = "N" * min(rng.choice([1, 2, 31, 32, 33, 90]), n - p)
        recs.append((f"r{r}", "".join(s)[:n]))
    recs.append(("long", "".join(rng.choice("ACGT") for _ in range(150000))))
    st = _check(oracle, recs, 32, 200)
    assert st["bs_filter_bases"] > 0 or os.environ.get("MXG_BS") == "0"  # (MXG_BS=0: the rolling-hash route is under test)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_select_halo_where_runs_meet(oracle, env, seed):
    """records made of many valid runs between N gaps, run lengths just under / at / over whole strips and just under / over a
    window: the halo of a slice (strips on either side of its own ones) must still hold w k-mers of the contig where a run's
    short last strip falls into it (bs_select_halo), or the route must decline the assembly -- either way the sketch is the
    oracle's"""
    rng = random.Random(seed)
    S, w, k = 320, 1000, 32
    env["MXG_SPARSE_S"] = str(S)
    env["MXG_DEV_GAPS"] = "1"
    recs = []
    for r in range(6):
        parts = []
        for _ in range(rng.randrange(8, 40)):
            n_kmers = rng.choice([S - 1, S, S + 1, 2 * S - 1, 2 * S + 3, 3 * S, w - 2, w, w + 1, 5, 40, 4 * S + 7, rng.randrange(1, 6000)])
            parts.append("".join(rng.choice("ACGT") for _ in range(n_kmers + k - 1)))
            parts.append("N" * rng.choice([1, 1, 2, 31, 32, 33, 100]))
        recs.append((f"r{r}", "".join(parts)))
    recs.append(("plain", "".join(rng.choice("ACGT") for _ in range(120000))))
    st = _check(oracle, recs, k, w)
    st2 = _check(oracle, recs, k, w, cand_per_window=4)
    assert st["bs_filter_bases"] > 0 and st2["bs_filter_bases"] > 0


def test_knobs_are_read_once_per_handle_and_reported(oracle, env):
    """mxg_knobs: the MXG_* switches a handle read and found set, as it first saw them (a later change of the environment does
    not reach a handle that has already run)"""
    from ntjoin_amd.engine import MxEngine
    env["MXG_SPARSE_S"] = "128"
    env["MXG_BS_SELECT"] = "0"
    recs = _records(61)
    with MxEngine(k=32, w=200) as eng:
        eng.add_records("x", 1.0, recs)
        eng.sketch()
        first = eng.get_sketch(0)["out_hash"].copy()
        kn = dict(kv.split("=", 1) for kv in eng.knobs().split())
        assert kn.get("MXG_SPARSE_S") == "128" and kn.get("MXG_BS_SELECT") == "0"
        assert eng.stats()["select_slices"] == 0
        env["MXG_BS_SELECT"] = "1"     # too late for this handle
        eng.sketch()
        assert eng.stats()["select_slices"] == 0
        assert (eng.get_sketch(0)["out_hash"] == first).all()
    with MxEngine(k=32, w=200) as eng:
        eng.add_records("x", 1.0, recs)
        eng.sketch()
        assert eng.stats()["select_slices"] > 0 and "MXG_BS_SELECT=1" in eng.knobs()


def test_held_back_emit_places_what_an_emit_in_place_does(oracle, env):
    """Three single-batch assemblies on the slice route: the first two emits are held back and enqueued behind the NEXT assembly's
    slice kernel, the last one at the end of the step (MXG_DEFER_EMIT=0: every emit in its own place; MXG_STAGGER=0: no filter
    waits for a slice kernel, and nothing is held back).  MXG_DEV_GAPS=1, so that the placing blocks and the stretch capacity of
    a batch travel with its held emit; _records has N runs and low-complexity islands longer than the window, which make
    candidate-free stretches.  _records at w = 1000 is the smallest input on which this file asserts select_slices > 0
    (test_select_route_is_the_default_for_small_inputs).  Knobs are parsed once per handle: a fresh handle per setting."""
    from ntjoin_amd.engine import MxEngine
    w = 1000
    asms = [_records(700 + a) for a in range(3)]
    want = [_expected(oracle, recs, 32, w) for recs in asms]
    env["MXG_DEV_GAPS"] = "1"
    for knob, value in ((None, None), ("MXG_DEFER_EMIT", "0"), ("MXG_STAGGER", "0")):
        env.pop("MXG_DEFER_EMIT", None)
        env.pop("MXG_STAGGER", None)
        if knob:
            env[knob] = value
        with MxEngine(k=32, w=w) as eng:
            for a, recs in enumerate(asms):
                eng.add_records(f"asm{a}", 1.0, recs)
            eng.sketch()
            for a in range(len(asms)):
                _assert_sketch(eng.get_sketch(a), want[a], (knob, a))
            st = eng.stats()
            if knob:
                assert f"{knob}={value}" in eng.knobs().split(), "the handle did not read the knob"
        assert st["select_slices"] > 0, (knob, "k_bs_select did not run")


# ---------------------------------------------------------------------------------------------------------------
# the request array of k_sel_stretch at its capacity (MXG_SEL_IREQ_CAP = usable requests per batch; csrc/sel_requests.h)
# ---------------------------------------------------------------------------------------------------------------
IREQ_KNOB = "MXG_SEL_IREQ_CAP"
IREQ_USABLE = (1 << 18) - 8


def _expected(oracle, recs, k, w):
    """the oracle's sketch of every record, computed once per input: [(hash, position, strand)] per record"""
    return [[(h, p, f) for h, p, f, _ in oracle.sketch(seq, k, w, _oracle.V2_SUM)] for _, seq in recs]


def _assert_sketch(sk, want, ctx):
    """hash, position, strand and record borders, bit for bit; and, named on its own: no minimizer twice (what a stale request for
    k_sel_stretch does -- a stretch sketched into a row a second time -- in a batch that still ends well)"""
    first = sk["record_first"].tolist()
    borders = [0]
    for exp in want:
        borders.append(borders[-1] + len(exp))
    for r, exp in enumerate(want):
        lo, hi = int(first[r]), int(first[r + 1])
        pos = sk["pos"][lo:hi].tolist()
        assert len(set(pos)) == len(pos), ("a minimizer is duplicated", ctx, r)
        got = list(zip(sk["out_hash"][lo:hi].tolist(), pos, sk["forward"][lo:hi].tolist()))
        assert got == exp, (ctx, r)
    assert first == borders and len(sk["out_hash"]) == borders[-1], ctx


def _sketch_at_cap(env, recs, w, c, cap, want, ctx=None, calls=1):
    """one handle, `calls` sketches of recs with the request array's capacity forced to cap (None: as shipped) -> stats"""
    from ntjoin_amd.engine import MxEngine
    if cap is None:
        env.pop(IREQ_KNOB, None)
    else:
        env[IREQ_KNOB] = str(cap)
    with MxEngine(k=32, w=w, cand_per_window=c) as eng:
        eng.add_records("x", 1.0, recs)
        for call in range(calls):
            eng.sketch(-2)
            _assert_sketch(eng.get_sketch(0), want, (ctx, w, c, cap, call))
        st = eng.stats()
        if cap is not None:
            assert f"{IREQ_KNOB}={cap}" in eng.knobs().split(), "the handle did not read the knob"
    return st


def _once(st):
    """every batch was enqueued and summed up once: the statistics are then sums over the batches as they ran"""
    return st["batches_redone"] == 0 and st["retried_assemblies"] == 0 and st["sync_assemblies"] == 0


def _iid(seed, n):
    rng = random.Random(seed)
    return "".join(rng.choice("ACGT") for _ in range(n))


@pytest.mark.parametrize("dev_gaps", ["0", "1"])
def test_request_capacity_every_cap_of_a_small_input(oracle, env, dev_gaps):
    """one i.i.d. record of 200 kbp at (w = 64, c = 2), strips of 320: every slice holds far more than SEL_REQ = 8 stretches between
    two of its candidates, so nearly every slice reserves eight requests: R = slice_stretches > L = select_slices without the
    knob, and some slice holds at least two requests.  Reservations are contiguous, so among the capacities 1 .. R + 1 some fall
    strictly inside a reservation of several requests, whatever order the adds landed in: the cut reservation (tombstones in front
    of the capacity, all of the slice's stretches to k_gap_fix) is exercised for certain, as are the exact fit and the capacities
    one entry either side of it.  The counter goes on counting at the capacity; the statistic is what the array took.
    Measured on an MI355X: R = 87, L = 11 (ten slices with eight requests, one with seven), with and without MXG_DEV_GAPS; with
    MXG_DEV_GAPS=1 every batch is enqueued once and the statistic is exact at all 88 capacities."""
    recs = [("iid", _iid(4242, 200_000))]
    env["MXG_SPARSE_S"] = "320"
    env["MXG_DEV_GAPS"] = dev_gaps
    want = _expected(oracle, recs, 32, 64)
    st0 = _sketch_at_cap(env, recs, 64, 2, None, want)
    R, L = st0["slice_stretches"], st0["select_slices"]
    print(f"request capacity sweep (dev_gaps={dev_gaps}): R = {R} requests, L = {L} slices")
    assert R > L > 0, (R, L)
    assert R <= 600, R               # (a sweep of a few hundred handles; a larger R wants a shorter record)
    exact = 0
    for cap in range(1, R + 2):
        st = _sketch_at_cap(env, recs, 64, 2, cap, want)
        assert 0 < st["slice_stretches"] and st["select_slices"] >= L, cap
        if _once(st0) and _once(st):   # (one record is one batch: its array took min(R, cap) entries)
            assert st["slice_stretches"] == min(R, cap) and st["select_slices"] == L, (cap, st["slice_stretches"])
            exact += 1
    print(f"request capacity sweep (dev_gaps={dev_gaps}): {exact} of {R + 1} capacities with every batch enqueued once")


def _several_records(seed, lengths):
    rng = random.Random(seed)
    return [(f"r{i}", "".join(rng.choice("ACGT") for _ in range(n))) for i, n in enumerate(lengths)]


def test_request_capacity_stale_requests_of_earlier_batches(oracle, env):
    """the array is never cleared: what a batch leaves in it -- requests in front of the capacity, untouched entries behind a cut
    reservation until this was fixed -- is there when the next batch of the handle walks its min(counter, capacity) entries.
    Batches are whole records: with a budget of 50 000 k-mers each of the six records of 40 to 90 kbp is a batch of its own (no
    two fit one budget; more slices than the unforced run makes says that the budget took).  Two sketches per handle, capacities
    3, 11 and half of what an average batch asks for; then a handle that sketches assembly A, and then A and another assembly B
    of other record lengths, whose batches walk what A's left."""
    from ntjoin_amd.engine import MxEngine
    env["MXG_SPARSE_S"] = "320"
    env["MXG_DEV_GAPS"] = "1"
    w, c, budget = 64, 2, 50_000
    recs_a = _several_records(91, [90_000, 40_000, 75_000, 55_000, 60_000, 41_000])
    recs_b = _several_records(92, [30_000, 120_000, 47_000, 83_000, 52_000])
    want_a, want_b = _expected(oracle, recs_a, 32, w), _expected(oracle, recs_b, 32, w)
    one = _sketch_at_cap(env, recs_a, w, c, None, want_a, "one batch")
    env["MXG_SPARSE_BATCH_KMERS"] = str(budget)
    st = _sketch_at_cap(env, recs_a, w, c, None, want_a, "batches")
    assert st["select_slices"] > one["select_slices"], "one batch: MXG_SPARSE_BATCH_KMERS did not take"
    assert all(len(x) + len(y) - 62 > budget for (_, x), (_, y) in zip(recs_a, recs_a[1:]))
    n_batches = len(recs_a)
    multi = st["slice_stretches"]
    R = multi // n_batches
    print(f"stale requests: {st['slice_stretches']} requests in {n_batches} batches, {st['select_slices']} slices ({one['select_slices']} in one batch)")
    assert n_batches >= 4 and R // 2 > 11
    for cap in (3, 11, R // 2):
        st = _sketch_at_cap(env, recs_a, w, c, cap, want_a, "two sketches of a handle", calls=2)
        assert 0 < st["slice_stretches"] <= 2 * multi, cap   # (two sketches of the handle, every batch's count bounded by the capacity)
        env[IREQ_KNOB] = str(cap)
        with MxEngine(k=32, w=w, cand_per_window=c) as eng:
            eng.add_records("a", 1.0, recs_a)
            eng.sketch(-2)
            _assert_sketch(eng.get_sketch(0), want_a, ("A alone", cap))
            eng.add_records("b", 1.0, recs_b)
            eng.sketch(-2)
            _assert_sketch(eng.get_sketch(0), want_a, ("A beside B", cap))
            _assert_sketch(eng.get_sketch(1), want_b, ("B behind A", cap))


def _stretch_records():
    """the records of test_stretches_are_sketched_behind_the_slice_kernel and of test_select_stretch_ends_behind_the_slice"""
    rng = random.Random(77)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    plain = [("a", rnd(700000)), ("b", rnd(1500)), ("c", rnd(1031)), ("d", rnd(300000)), ("n_inside", rnd(40000) + "N" + rnd(50000) + "NNNN" + rnd(800)),
             ("e", rnd(2200)), ("f", rnd(450000))]
    rng = random.Random(5)
    unit = rnd(171)
    long_ = [("sat", rnd(30000) + unit * 400 + rnd(30000)), ("polyA", rnd(5000) + "A" * 90000 + rnd(2000)),
             ("unit7", ("ACGGTCA" * 20000)[:100000]), ("plain", rnd(200000)), ("polyT_end", rnd(3000) + "T" * 50000)]
    return {"between_candidates": plain, "behind_the_slice": long_}


@pytest.mark.parametrize("which", ["between_candidates", "behind_the_slice"])
@pytest.mark.parametrize("w,c", [(1000, 4), (300, 3), (2500, 3), (64, 2)])
def test_request_capacity_realistic_shapes(oracle, env, which, w, c):
    """stretches between two candidates of a slice, at a contig's start and end, across N, taken in pieces (w = 2500), and stretches
    that end far behind the slice: capacities 1, 8, 9 (one request, one full reservation, one more), half of what the input
    asks for, one less than that, exactly that (the last reservation fits exactly: nothing falls back)"""
    recs = _stretch_records()[which]
    env["MXG_SPARSE_S"] = "320"
    env["MXG_DEV_GAPS"] = "1"
    want = _expected(oracle, recs, 32, w)
    st0 = _sketch_at_cap(env, recs, w, c, None, want, which)
    R = st0["slice_stretches"]
    print(f"realistic shapes {which} w={w} c={c}: R = {R} requests, {st0['select_slices']} slices")
    assert R > 5 and st0["select_slices"] > 0, R
    for cap in sorted({1, 8, 9, max(1, R // 2), R - 1, R}):
        st = _sketch_at_cap(env, recs, w, c, cap, want, which)
        # (the records may make several batches, each with an array of its own: every batch's count is bounded by the capacity)
        assert 0 < st["slice_stretches"] and (st["slice_stretches"] <= R or not (_once(st0) and _once(st))), (cap, st["slice_stretches"])
    if _once(st0) and _once(st):     # (capacity R binds in no batch: as without the knob)
        for key in ("slice_stretches", "deferred_stretches", "dense_kmers"):
            assert st[key] == st0[key], key


def test_request_capacity_fused_call(oracle, env, tmp_path):
    """mxg_sketch_graph at a capacity of nine requests (every batch cuts a reservation) against mxg_sketch + mxg_build_graph of the
    same two assemblies at the same capacity, and against both without the knob: sketches, minimizer flags, canonical .mx.dot"""
    import numpy as np
    from ntjoin_amd.engine import MxEngine
    from oracle import graph_oracle
    env["MXG_SPARSE_S"] = "320"
    env["MXG_DEV_GAPS"] = "1"
    w, c = 300, 3
    ref = _stretch_records()["between_candidates"]
    comp = str.maketrans("ACGT", "TGCA")
    tgt = [(f"t{i}", s[::-1].translate(comp) if i % 2 else s) for i, (_, s) in enumerate(ref) if "N" not in s][::-1]
    want = [_expected(oracle, recs, 32, w) for recs in (ref, tgt)]
    res = {}
    for cap in (None, 9):
        for fused in (False, True):
            if cap is None:
                env.pop(IREQ_KNOB, None)
            else:
                env[IREQ_KNOB] = str(cap)
            with MxEngine(k=32, w=w, cand_per_window=c) as eng:
                eng.add_records("ref.fa.k32.w300.tsv", 2.0, ref)
                eng.add_records("tgt.fa.k32.w300.tsv", 1.0, tgt)
                if fused:
                    eng.sketch_graph()
                else:
                    eng.sketch(-2)
                    eng.build_graph()
                for a in range(2):
                    _assert_sketch(eng.get_sketch(a), want[a], ("fused" if fused else "two calls", cap, a))
                dot = str(tmp_path / f"{cap}_{fused}.mx.dot")
                eng.write_dot(dot)
                with open(dot, encoding="utf-8") as fh:
                    res[cap, fused] = (graph_oracle.canonical_dot_from_text(fh.read()), [eng.get_mx_flags(a).copy() for a in range(2)],
                                       eng.stats())
    base = res[None, False]
    assert base[2]["slice_stretches"] > 100    # (hundreds of requests: a capacity of nine binds in every batch)
    for key, (dot, flags, st) in res.items():
        assert dot == base[0], key
        assert all(np.array_equal(x, y) for x, y in zip(flags, base[1])), key
        if _once(st) and _once(base[2]):   # (nine requests per batch's array, however many batches)
            assert st["slice_stretches"] == base[2]["slice_stretches"] if key[0] is None else 0 < st["slice_stretches"] < base[2]["slice_stretches"], key


def test_request_capacity_that_does_not_bind(oracle, env):
    """a capacity of what the input asks for, of more, of more than the array has (clamped to its 262 136 usable entries):
    statistics and sketch are those of a run without the knob"""
    recs = [("iid", _iid(4243, 150_000)), ("short", _iid(4244, 1200))]
    env["MXG_SPARSE_S"] = "320"
    env["MXG_DEV_GAPS"] = "1"
    want = _expected(oracle, recs, 32, 64)
    st0 = _sketch_at_cap(env, recs, 64, 2, None, want)
    R = st0["slice_stretches"]
    assert R > 8
    for cap in (R, R + 1, 4 * R, IREQ_USABLE, 10 ** 9):
        st = _sketch_at_cap(env, recs, 64, 2, cap, want)
        for key in ("slice_stretches", "select_slices", "candidates", "dense_kmers", "deferred_stretches", "batches_redone", "minimizers"):
            assert st[key] == st0[key], (cap, key)
