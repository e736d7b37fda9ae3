"""GPU test of the learnt verdict prefill of assembly 0 (PJ_PREFILL_OWN0, join_verdict.h) when its guess is WRONG.

A handle that found more than half of assembly 0 shared plans its next build of the same sizes with the prefill "shared, a vertex,
own index" for assembly 0 (JoinLearnt::prefill_own0, join_plan.h).  The guess is keyed by the sizes alone, and a sketch can be
replaced on a live handle without changing them.  The contract is that the result is right whatever the guess; every other test
that reaches prefill0=1 builds the same minimizers twice, so the guess it sees is right.

The route here: a TEACHER of the case's sizes (assembly a = the first n_a keys of one pool of max(n) distinct keys: the smallest
assembly is shared whole) is added and built, every assembly's sketch is then replaced by the case's arrays
(MxEngine.set_sketch_device), and the graph is built again.  That build must say prefill0=1 on its MXG_DEBUG_JOIN line and give
the case's own reference: flags from numpy, vertices and edges from the C oracle, every array equal to a fresh handle's
global-table build.  Two conditions are checked on the CPU at import, so that no case passes empty: the teacher teaches
(2 min(n_a) > n_0 and more than half of its assembly 0 shared), and the case has at most half of assembly 0 shared, with every
kind of verdict on its list IN ASSEMBLY 0, where the rule acts."""
import numpy as np
import pytest

from tests.test_gpu_join_records import CASES as RECORD_CASES
from tests.test_gpu_join_records import KNOBS, R12, _join_lines, _reference
from tests.test_gpu_join_verdicts import CASES as VERDICT_CASES
from tests.test_gpu_join_verdicts import DUP, DUP_INALL, ONCE_HERE, SHARED, SKIPPED, _asm, _check, _keys, _state, _thirds, _truth

pytestmark = pytest.mark.gpu

# every two-level route and the bytes of its records
ROUTES = {
    "12 bytes": (R12, 12),
    "skew path": (dict(R12, MXG_PJ_SKEW="1"), 12),
    "16 bytes": ({"MXG_PJ_TWO_LEVEL": "1"}, 16),
    "plain join kernel": (dict(R12, MXG_PJ_PIPE="0"), 16),
    "REC12=0": (dict(R12, MXG_PJ_REC12="0"), 16),
}
TWO_ROUTES = ("12 bytes", "16 bytes")


def _sizes(sets):
    return tuple(int(s[0].size) for s in sets)


def _shared0(sets):
    f0 = _truth(sets)[0]
    return int((f0 == SHARED).sum()), int(f0.size)


_TEACHERS = {}


def _teacher(sizes):
    """assembly a = the first n_a keys of one pool of max(n) distinct keys, shuffled per assembly: the keys of the smallest assembly
    are once in every assembly.  It teaches the rule only if that is more than half of assembly 0."""
    sizes = tuple(sizes)
    if sizes not in _TEACHERS:
        rng = np.random.default_rng([40, len(sizes), sizes[0]])
        pool = _keys(rng, max(sizes))
        assert np.unique(pool).size == pool.size
        sets = []
        for n in sizes:
            hs = pool[:n].copy()
            rng.shuffle(hs)
            sets.append(_asm(hs))
        shared0, n0 = _shared0(sets)
        assert 2 * min(sizes) > sizes[0] and shared0 == min(sizes) and 2 * shared0 > n0, f"the teacher of {sizes} teaches nothing"
        _TEACHERS[sizes] = sets
    return _TEACHERS[sizes]


def _wrong_guess(name, sets, kinds0=()):
    """the case as the tests use it; refused at import unless the teacher of its sizes teaches, at most half of its assembly 0 is
    shared, and every kind on its list occurs in assembly 0"""
    _teacher(_sizes(sets))
    f0 = _truth(sets)[0]
    assert 2 * int((f0 == SHARED).sum()) <= f0.size, f"case '{name}': the guess would be right"
    for kind in kinds0:
        assert (f0 == kind).any(), f"case '{name}' has no verdict of kind {kind} in assembly 0"
    return sets


def _padded(sets, seed, pad0=0):
    """the other assemblies padded with private keys until the teacher of these sizes teaches (2 n_a > n_0); assembly 0 keeps its
    order (pad0 private keys go behind it), the others are shuffled again"""
    rng = np.random.default_rng(seed)
    hs0 = np.concatenate([sets[0][0], _keys(rng, pad0)])
    out = [_asm(hs0)]
    for s in sets[1:]:
        hs = np.concatenate([s[0], _keys(rng, max(0, hs0.size // 2 + 1 - s[0].size))])
        rng.shuffle(hs)
        out.append(_asm(hs))
    return out


def _with_once_here(sets, at, seed):
    """fresh keys once in assembly 0 (at the given indices), twice in assembly 1 and once in every other assembly: ONCE_HERE in
    assembly 0"""
    rng = np.random.default_rng(seed)
    keys = _keys(rng, len(at))
    hs0 = sets[0][0].copy()
    hs0[np.asarray(at)] = keys
    out = [_asm(hs0)]
    for a, s in enumerate(sets[1:], start=1):
        hs = np.concatenate([s[0], keys, keys] if a == 1 else [s[0], keys])
        rng.shuffle(hs)
        out.append(_asm(hs))
    return out


def _runs_to_the_end(sets, seed):
    """the "runs" case with 100 minimizers more in assembly 0 (its last 256-block is partial) and a run of 140 equal hashes from
    index 6616 to the last element: over the border of the last whole 256-block, up to the array's end.  Its key lies once in the
    two other assemblies: every follower's prefill claims SHARED where the leader's word says DUP_INALL."""
    rng = np.random.default_rng(seed)
    n0 = sets[0][0].size
    assert n0 % 256 == 0
    key = _keys(rng, 1)
    hs0 = np.concatenate([sets[0][0], _keys(rng, 100)])
    hs0[n0 - 40:] = key[0]
    out = [_asm(hs0)]
    for s in sets[1:]:
        hs = np.concatenate([s[0], key])
        rng.shuffle(hs)
        out.append(_asm(hs))
    return out


# ---- the verdict matrix of test_gpu_join_verdicts.py under a wrong guess ----------------------------------------------------------
# ("special keys": 505 of its 994 minimizers of assembly 0 are shared; 100 private keys behind them bring that below half.
# "runs" and "heavy key" have ONCE_HERE in the other assemblies only: five keys once in assembly 0 and twice in assembly 1 are added,
# at indices that no run and no copy of the heavy key occupies.)
MATRIX = {
    "thirds 3000+2500": (_padded(VERDICT_CASES["thirds 3000+2500"][0], 51), (SKIPPED, SHARED, DUP)),
    "two of three": (_padded(VERDICT_CASES["two of three"][0], 52), (SKIPPED, SHARED)),
    "runs": (_padded(_with_once_here(_runs_to_the_end(VERDICT_CASES["runs"][0], 53), range(6600, 6605), 54), 55),
             (SKIPPED, SHARED, DUP, DUP_INALL, ONCE_HERE)),
    "special keys": (_padded(VERDICT_CASES["special keys"][0], 56, pad0=100), (SKIPPED, SHARED, DUP)),
    "heavy key": (_padded(_with_once_here(VERDICT_CASES["heavy key"][0], range(20000, 20005), 57), 58),
                  (SKIPPED, SHARED, DUP_INALL, ONCE_HERE)),
}
for _name, (_sets, _kinds) in MATRIX.items():
    _wrong_guess(_name, _sets, _kinds)
    assert max(_sizes(_sets)) <= 30000
assert _sizes(MATRIX["runs"][0])[0] % 256 == 100 and (MATRIX["runs"][0][0][0][-140:] == MATRIX["runs"][0][0][0][-1]).all()


def _session(monkeypatch, capfd, env, first, script):
    """One handle under `env`: `first` goes in through add_minimizers and is built; for every entry of `script` every assembly's
    sketch is replaced by the entry's arrays (None: nothing is replaced) and the graph is built again.
    -> [(state, graph_join, the [mxg] join lines)] of every build"""
    import torch
    from ntjoin_amd.engine import MxEngine
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    for key, val in dict(env, MXG_DEBUG_JOIN="1").items():  # (knobs are read once per handle: set before it exists)
        monkeypatch.setenv(key, val)
    out = []
    with MxEngine(k=32, w=1000) as eng:
        for a, (hs, pos, rec, ids) in enumerate(first):
            eng.add_minimizers(f"a{a}", 1.0 + a / 4, hs, pos, rec, ids)
        for sets in [None] + list(script):
            if sets is not None:
                assert len(sets) == len(first)
                for a, (hs, pos, rec, _) in enumerate(sets):
                    dev = [torch.from_numpy(np.ascontiguousarray(x).view(t)).cuda() for x, t in ((hs, np.int64), (pos, np.int32), (rec, np.int32))]
                    eng.set_sketch_device(a, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), None, hs.size)
            capfd.readouterr()
            eng.build_graph()
            lines = _join_lines(capfd.readouterr().err)
            out.append((_state(eng, len(first)), int(eng.stats()["graph_join"]), lines))
    return out


def _one_attempt(lines, nbytes, prefill0):
    assert len(lines) == 1, lines
    for key, val in dict(pj=1, two_level=1, record_bytes=nbytes, prefill0=prefill0).items():
        assert lines[0][key] == val, (key, lines[0])


def _stale_build(monkeypatch, capfd, route, sets):
    """the teacher, then the swap: -> the state of the build that ran under the wrong guess (prefill0=1 asserted)"""
    env, nbytes = ROUTES[route]
    (_, join_t, lines_t), (state, join, lines) = _session(monkeypatch, capfd, env, _teacher(_sizes(sets)), [sets])
    assert join_t == 2 and join == 2, (hex(join_t), hex(join))
    _one_attempt(lines_t, nbytes, 0)
    _one_attempt(lines, nbytes, 1)
    return state


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", list(MATRIX))
def test_verdict_matrix_under_a_wrong_guess(name, route, monkeypatch, capfd):
    """every kind of verdict in assembly 0 where the prefill claims SHARED: word 1 is sent, followers drop their prefill for the
    leader's word, the skew path's references resolve to a word that is no prefill"""
    sets = MATRIX[name][0]
    ref = _reference(monkeypatch, capfd, "stale " + name, sets)
    _check(_stale_build(monkeypatch, capfd, route, sets), ref, (name, route))


@pytest.mark.parametrize("route", TWO_ROUTES)
def test_other_sizes_forget_the_guess(route, monkeypatch, capfd):
    """the control: one minimizer more in assembly 1 than the teacher had, and the build keeps today's prefill"""
    sets = _thirds([3000, 2501], 11)
    env, nbytes = ROUTES[route]
    ref = _reference(monkeypatch, capfd, "stale control", sets)
    (_, _, lines_t), (state, join, lines) = _session(monkeypatch, capfd, env, _teacher((3000, 2500)), [sets])
    _one_attempt(lines_t, nbytes, 0)
    _one_attempt(lines, nbytes, 0)
    assert join == 2, hex(join)
    _check(state, ref, route)


def _nothing_shared(seed):
    rng = np.random.default_rng(seed)
    return [_asm(_keys(rng, 2000)), _asm(_keys(rng, 2500))]


NOTHING = _wrong_guess("nothing shared", _nothing_shared(61), (SKIPPED,))


def test_nothing_shared(monkeypatch, capfd):
    """assembly 0 shares no key with assembly 1: every word of assembly 0 is word 1 and has to be sent; no vertex, no edge, and
    equal (zero) shared counts in both assemblies (the build would raise otherwise)"""
    ref = _reference(monkeypatch, capfd, "stale nothing shared", NOTHING)
    state = _stale_build(monkeypatch, capfd, "12 bytes", NOTHING)
    assert state["vertex_hash"].size == 0 and state["edge_u"].size == 0
    assert (state["flags0"] == SKIPPED).all() and (state["flags1"] == SKIPPED).all()
    _check(state, ref, "nothing shared")


# ---- the smallest shapes ------------------------------------------------------------------------------------------------------
def _smallest(n0, kind, seed):
    """n_1 = n_0 + 3.  The even-indexed minimizers of assembly 0 are shared and the odd ones private, then the LAST index gets a
    minimizer of `kind` (a duplicate's twin sits at index 1, not beside it: no run), and where that leaves more than half of
    assembly 0 shared the lowest shared indices turn private: the shared share sits at half or just below."""
    rng = np.random.default_rng([seed, n0, kind])
    hs0 = _keys(rng, n0)
    last = n0 - 1
    shared = set(range(0, n0, 2)) - {last}
    extra = []
    if kind == SHARED:
        shared.add(last)
    elif kind in (DUP, DUP_INALL):
        hs0[last] = hs0[1]
        extra = [hs0[1]] if kind == DUP_INALL else []
    elif kind == ONCE_HERE:
        extra = [hs0[last]] * 2
    while 2 * len(shared) > n0:
        shared.remove(min(shared - {last}))
    in1 = np.array([hs0[i] for i in sorted(shared)] + extra, dtype=np.uint64)
    hs1 = np.concatenate([in1, _keys(rng, n0 + 3 - in1.size)])
    rng.shuffle(hs1)
    return [_asm(hs0), _asm(hs1)]


SMALLEST = {}
for _n0 in (1, 63, 64, 65, 255, 256, 257):
    # (one minimizer can be neither a duplicate nor, below half, shared)
    for _kind in ((SKIPPED, ONCE_HERE) if _n0 == 1 else (SKIPPED, SHARED, DUP, DUP_INALL, ONCE_HERE)):
        _sets = _wrong_guess(f"smallest {_n0}/{_kind}", _smallest(_n0, _kind, 62))
        _f0 = _truth(_sets)[0]
        assert _sizes(_sets) == (_n0, _n0 + 3) and _f0[-1] == _kind
        assert _n0 // 2 - 1 <= int((_f0 == SHARED).sum()) <= _n0 // 2
        SMALLEST[(_n0, _kind)] = _sets


@pytest.mark.parametrize("n0,kind", list(SMALLEST))
def test_smallest_shapes(n0, kind, monkeypatch, capfd):
    """n_0 around a wave and a 256-block, the teacher fully shared, the case shared at every other index, one minimizer of each
    kind at the last index"""
    sets = SMALLEST[(n0, kind)]
    ref = _reference(monkeypatch, capfd, f"stale smallest {n0}/{kind}", sets)
    for route in TWO_ROUTES:
        _check(_stale_build(monkeypatch, capfd, route, sets), ref, (n0, kind, route))


# ---- one assembly alone -----------------------------------------------------------------------------------------------------------
def _all_twice(n, seed):
    rng = np.random.default_rng(seed)
    half = _keys(rng, n // 2)
    hs = np.concatenate([half, half])
    rng.shuffle(hs)
    return [_asm(hs)]


ALONE = VERDICT_CASES["one assembly"][0]
ALONE_TWICE = _all_twice(ALONE[0][0].size, 63)
assert _sizes(ALONE) == _sizes(ALONE_TWICE) and 2 * _shared0(ALONE)[0] > _shared0(ALONE)[1]
assert (_truth(ALONE_TWICE)[0] == DUP_INALL).all()


@pytest.mark.parametrize("route", list(ROUTES))
def test_one_assembly_alone(route, monkeypatch, capfd):
    """with one assembly every key that occurs once is shared: the data teaches by being built twice; then every key occurs twice
    -- no vertex, every flag DUP_INALL, under a prefill that claims a vertex for every minimizer"""
    env, nbytes = ROUTES[route]
    ref = _reference(monkeypatch, capfd, "stale alone", ALONE)
    ref_twice = _reference(monkeypatch, capfd, "stale alone twice", ALONE_TWICE)
    builds = _session(monkeypatch, capfd, env, ALONE, [None, ALONE_TWICE])
    for b, (state, join, lines) in enumerate(builds):
        assert join == 2, (b, hex(join))
        _one_attempt(lines, nbytes, 1 if b else 0)
        _check(state, ref_twice if b == 2 else ref, (route, b))
    assert builds[2][0]["vertex_hash"].size == 0 and (builds[2][0]["flags0"] == DUP_INALL).all()


# ---- 32 assemblies: the wide kernels ------------------------------------------------------------------------------------------
def _two_thirds(sizes, seed):
    """two thirds of the smallest assembly's keys in every assembly, the rest their own, some twice"""
    rng = np.random.default_rng(seed)
    common = _keys(rng, 2 * min(sizes) // 3)
    sets = []
    for n in sizes:
        twice = _keys(rng, min(sizes) // 12)
        hs = np.concatenate([common, _keys(rng, n - common.size - 2 * twice.size), twice, twice])
        rng.shuffle(hs)
        sets.append(_asm(hs))
    return sets


WIDE = _wrong_guess("32 assemblies", RECORD_CASES["32 assemblies"], (SKIPPED, SHARED, DUP))
WIDE_RIGHT = _two_thirds(_sizes(WIDE), 64)
assert len(WIDE) == 32 and _sizes(WIDE)[0] == min(_sizes(WIDE)) and 2 * _shared0(WIDE_RIGHT)[0] > _shared0(WIDE_RIGHT)[1]


@pytest.mark.parametrize("route", list(ROUTES))
def test_32_assemblies(route, monkeypatch, capfd):
    """more than 16 assemblies (the kernels whose seen and dup masks have a word each): a stale guess after the teacher, then a
    right one -- two builds of a set with two thirds of assembly 0 shared"""
    env, nbytes = ROUTES[route]
    _check(_stale_build(monkeypatch, capfd, route, WIDE), _reference(monkeypatch, capfd, "stale 32", WIDE), (route, "stale"))
    ref = _reference(monkeypatch, capfd, "stale 32 right", WIDE_RIGHT)
    for b, (state, join, lines) in enumerate(_session(monkeypatch, capfd, env, WIDE_RIGHT, [None])):
        assert join == 2, (b, hex(join))
        _one_attempt(lines, nbytes, b)
        _check(state, ref, (route, "right", b))


# ---- the redo with the global table, the guess that flips back --------------------------------------------------------------------
def test_redo_with_the_global_table_under_a_wrong_guess(monkeypatch, capfd):
    """MXG_PJ_FORCE_FAIL=1 from the start: the teacher's build ends in the global table and still records its count; the swap
    (set_sketch_device forgets the overflow, JoinLearnt::sketch_replaced, and keeps the guess) lets the next build try the LDS join
    first, under prefill0=1, before it fails again and the global table redoes it over slots that hold the stale prefill"""
    name = "thirds 3000+2500"
    sets = MATRIX[name][0]
    ref = _reference(monkeypatch, capfd, "stale " + name, sets)
    env = {"MXG_PJ_TWO_LEVEL": "1", "MXG_PJ_FORCE_FAIL": "1"}
    (state_t, join_t, lines_t), (state, join, lines) = _session(monkeypatch, capfd, env, _teacher(_sizes(sets)), [sets])
    assert join_t & 0xFF == 3 and [ln["pj"] for ln in lines_t] == [1, 0] and lines_t[0]["prefill0"] == 0, (hex(join_t), lines_t)
    assert state_t["vertex_hash"].size == min(_sizes(sets))
    assert [ln["pj"] for ln in lines] == [1, 0], lines
    assert lines[0]["two_level"] == 1 and lines[0]["prefill0"] == 1, lines[0]
    assert join & 0xFF == 3, hex(join)
    _check(state, ref, "redo")


@pytest.mark.parametrize("route", TWO_ROUTES)
def test_the_guess_flips_back(route, monkeypatch, capfd):
    """teacher, the swapped case, the same case again: the second build runs under the wrong guess and corrects it, the third is
    back to today's prefill; both give the same arrays"""
    name = "thirds 3000+2500"
    sets = MATRIX[name][0]
    env, nbytes = ROUTES[route]
    ref = _reference(monkeypatch, capfd, "stale " + name, sets)
    builds = _session(monkeypatch, capfd, env, _teacher(_sizes(sets)), [sets, None])
    for (state, join, lines), prefill0 in zip(builds, (0, 1, 0)):
        assert join == 2, hex(join)
        _one_attempt(lines, nbytes, prefill0)
    _check(builds[1][0], ref, (route, "second"))
    _check(builds[2][0], ref, (route, "third"))
    assert builds[1][0].keys() == builds[2][0].keys()
    for key in builds[1][0]:
        assert np.array_equal(builds[1][0][key], builds[2][0][key]), key


# ---- the fused call: a borrowed buffer refilled -------------------------------------------------------------------------------
def test_fused_call_after_a_refill(monkeypatch, capfd):
    """mxg_sketch_graph needs no set_sketch_* to meet a stale guess.  A 2 Mbp reference and a target derived from it with 0.1 %
    substitutions, in borrowed device buffers, at w = 200: the fused call's key is its bounds (2.3 k-mers per window + 2048, the
    record layout alone: ~24 900 for ~19 900 minimizers) and it learns the rule if the shared minimizers of assembly 0 are more
    than half of that BOUND, which this pair clears.  Two calls (prefill0 = 0, then 1 with a right guess), then both buffers are
    overwritten in place with two independent random genomes of the same record lengths -- the same bounds, nothing shared -- and
    the third call runs early, under prefill0=1, and must give the flags of numpy and the state of a fresh global-table handle."""
    import torch
    from ntjoin_amd import synth
    from ntjoin_amd.engine import MxEngine
    ref = synth.make_reference(3, 2_000_000, 1)
    tgt = synth.derive_target(ref, 4, sub_rate=0.001)
    rng = np.random.default_rng(65)
    second = [[rng.integers(0, 4, size=len(r), dtype=np.uint8) for r in recs] for recs in (ref, tgt)]

    def add(eng, pairs):
        kept = []
        for (name, wt), recs in zip((("ref", 2.0), ("tgt", 1.0)), pairs):
            words, starts, lens = synth.pack_records(recs)
            d = torch.from_numpy(words.view(np.int32)).cuda()
            eng.add_packed_device(name, wt, d.data_ptr(), starts, lens, keepalive=d)
            kept.append(d)
        return kept

    def env_is(env):
        for key in KNOBS:
            monkeypatch.delenv(key, raising=False)
        for key, val in env.items():
            monkeypatch.setenv(key, val)

    def call(eng):
        capfd.readouterr()
        eng.sketch_graph()
        return _join_lines(capfd.readouterr().err), int(eng.stats()["graph_join"])

    env_is({"MXG_PJ_TWO_LEVEL": "1", "MXG_DEBUG_JOIN": "1"})
    with MxEngine(k=32, w=200) as eng:
        kept = add(eng, (ref, tgt))
        for want in (0, 1):
            lines, join = call(eng)
            assert join == 2 | 0x400 and len(lines) == 1 and lines[0]["early"] == 1 and lines[0]["prefill0"] == want, (want, hex(join), lines)
        shared0 = int((eng.get_mx_flags(0) == SHARED).sum())
        n0 = eng.get_mx_flags(0).size
        assert 2 * shared0 > 2.3 * (2_000_000 - 31) / 201 + 2048 > n0, (shared0, n0)  # (more than half of the bound)
        for d, recs in zip(kept, second):
            words, _, _ = synth.pack_records(recs)
            assert words.size == d.numel()
            d.copy_(torch.from_numpy(words.view(np.int32)))
        torch.cuda.synchronize()
        lines, join = call(eng)
        assert len(lines) == 1 and lines[0]["prefill0"] == 1 and lines[0]["early"] == 1 and lines[0]["two_level"] == 1, lines
        assert join == 2 | 0x400, hex(join)
        hashes = [np.array(eng.get_sketch(a)["out_hash"], copy=True) for a in range(2)]
        stale = _state(eng, 2)
    truth = _truth([(h,) for h in hashes])
    assert 2 * int((truth[0] == SHARED).sum()) <= truth[0].size and (truth[0] == SKIPPED).any()  # the guess was wrong
    for a in range(2):
        assert np.array_equal(stale[f"flags{a}"], truth[a]), a
    env_is({"MXG_GRAPH_JOIN": "global"})
    with MxEngine(k=32, w=200) as eng:
        add(eng, second)
        eng.sketch_graph()
        assert int(eng.stats()["graph_join"]) & 0xFF == 3
        for a in range(2):
            assert np.array_equal(eng.get_sketch(a)["out_hash"], hashes[a]), a
        fresh = _state(eng, 2)
    assert stale.keys() == fresh.keys()
    for key in stale:
        assert np.array_equal(stale[key], fresh[key]), key
