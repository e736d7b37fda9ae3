"""GPU test of the two-level join's 12-byte records and of the learnt verdict prefill of assembly 0 (join_plan.h, join_verdict.h).
Minimizer lists go in through add_minimizers with crafted hashes; every build must give the flags numpy gives, the vertices and
edges of the C oracle (oracle/graph_oracle.py's library) and the state of the global-table join.

The route.  12-byte records need two levels AND a sub-range per assembly in every coarse partition, which only the fused call
lays out by itself.  MXG_PJ_TWO_LEVEL=1 forces two levels at these sizes (P1 = 2 coarse x P = 256 fine partitions: 9 implied bits),
MXG_PJ_SPLIT=1 gives the stage's own plan the sub-ranges.  Every two-level shape with sub-ranges implies at least 6 bits
(P1 >= 2, P = 256), so "just below the condition" are the shapes that lack one of the other conditions: no sub-ranges, the plain
join kernel (MXG_PJ_PIPE=0), or MXG_PJ_REC12=0.  Which record and which prefill a build took is read from the line MXG_DEBUG_JOIN=1
prints per attempt (mxg_stats::graph_join has no bit for them)."""
import re

import numpy as np
import pytest

from tests import _oracle
from tests.test_gpu_join_verdicts import _asm, _check, _keys, _state, _truth

pytestmark = pytest.mark.gpu

KNOBS = ("MXG_GRAPH_JOIN", "MXG_PJ_TWO_LEVEL", "MXG_PJ_PIPE", "MXG_PJ_SKEW", "MXG_PJ_FORCE_FAIL", "MXG_PJ_EARLY", "MXG_PJ_SPLIT", "MXG_PJ_REC12",
         "MXG_PJ_PREFILL0", "MXG_DEBUG_JOIN")
R12 = {"MXG_PJ_TWO_LEVEL": "1", "MXG_PJ_SPLIT": "1"}
MUL = 0x9E3779B97F4A7C15
INV = pow(MUL, -1, 1 << 64)
ONES = (1 << 64) - 1
TAG_BITS = list(range(44, 50))          # P = 256: the tag takes the fine partition's six lowest bits
SAME_PART_BITS = [0, 31, 32, 42, 43, 53, 63]     # kept bits: a one-bit difference there leaves the record in its partition (P1 = 2: bit 52 is implied)


def _from_products(prods):
    return np.array([(int(p) * INV) & ONES for p in prods], dtype=np.uint64)


def _join_lines(err):
    """the [mxg] join lines of a build's stderr, one dict of numbers per attempt"""
    return [dict((k, int(v)) for k, v in re.findall(r"(\w+)=(\d+)", ln)) for ln in err.splitlines() if ln.startswith("[mxg] join")]


def _build(monkeypatch, capfd, sets, env, builds=1):
    """-> (state of every build, graph_join of every build, the [mxg] join lines of every build)"""
    from ntjoin_amd.engine import MxEngine
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    for key, val in dict(env, MXG_DEBUG_JOIN="1").items():
        monkeypatch.setenv(key, val)
    states, joins, lines = [], [], []
    with MxEngine(k=32, w=1000) as eng:
        for a, (hs, pos, rec, ids) in enumerate(sets):
            eng.add_minimizers(f"a{a}", 1.0 + a / 4, hs, pos, rec, ids)
        for _ in range(builds):
            capfd.readouterr()
            eng.build_graph()
            lines.append(_join_lines(capfd.readouterr().err))
            states.append(_state(eng, len(sets)))
            joins.append(int(eng.stats()["graph_join"]))
    return states, joins, lines


_REF = {}


def _reference(monkeypatch, capfd, name, sets):
    if name not in _REF:
        flags = _truth(sets)
        g = _oracle.load().graph([s[0] for s in sets], [s[2] for s in sets], [1.0 + a / 4 for a in range(len(sets))], edges=True)
        edges = sorted(zip(g["eu"].tolist(), g["ev"].tolist(), g["esup"].tolist(), g["ew"].tolist()))
        states, joins, _ = _build(monkeypatch, capfd, sets, {"MXG_GRAPH_JOIN": "global"})
        assert joins[0] & 0xFF == 3, hex(joins[0])
        _REF[name] = {"flags": flags, "vertices": g["vertices"], "edges": edges, "global": states[0]}
        _check(states[0], _REF[name], "global table")
    return _REF[name]


def _crafted(seed):
    """(a) for every tag bit t: products X and X ^ 2^t (equal in every kept bit, different fine partitions), X in both assemblies
    and the other in assembly 0 alone; for bits 50 and 51 likewise (implied but kept in the word).  For every kept bit that leaves
    the record where it is: X in assembly 0 alone, X ^ 2^bit in assembly 1 alone -- equal in all implied bits, one kept bit apart:
    a join that took them for one key would make a vertex of them."""
    rng = np.random.default_rng(seed)
    common = _keys(rng, 1500)
    only0, only1, both = [], [], []
    for j, bit in enumerate(TAG_BITS + [50, 51]):
        x = int(rng.integers(1, 2**63)) | (j << 8)
        both.append(x)
        only0.append(x ^ (1 << bit))
    for bit in SAME_PART_BITS:
        x = int(rng.integers(1, 2**63))
        only0.append(x)
        only1.append(x ^ (1 << bit))
        part = lambda p: ((p >> 44) & 255, (p >> 52) & 1)  # noqa: E731
        assert part(x) == part(x ^ (1 << bit))
    twice = _keys(rng, 200)
    hs0 = np.concatenate([common, _from_products(both), _from_products(only0), _keys(rng, 700), twice, twice])
    hs1 = np.concatenate([common, _from_products(both), _from_products(only1), _keys(rng, 431)])
    rng.shuffle(hs0)
    rng.shuffle(hs1)
    special = {"both": _from_products(both), "only0": _from_products(only0), "only1": _from_products(only1)}
    return [_asm(hs0), _asm(hs1)], special


def _thirds(sizes, seed):
    """a third of the smallest assembly's keys in every assembly, the rest their own, some twice"""
    rng = np.random.default_rng(seed)
    third = min(sizes) // 3
    common = _keys(rng, third)
    sets = []
    for n in sizes:
        twice = _keys(rng, third // 4)
        hs = np.concatenate([common, _keys(rng, n - third - 2 * twice.size), twice, twice])
        rng.shuffle(hs)
        sets.append(_asm(hs))
    return sets


def _heavy(seed):
    """(c) one key 8 000 times in assembly 0, never twice in a row, once in assembly 1, among 22 000 other keys (some of them
    twice).  Its coarse partition holds 11 000 + 8 000 records of assembly 0 against a mean of 15 000: above the skew limit
    (mean + mean / 32 + 2048 = 17 516), below the sub-range's capacity (24 576), so k_pj2_bucket's skew path runs by itself."""
    rng = np.random.default_rng(seed)
    common = _keys(rng, 6000)
    heavy = _keys(rng, 1)[0]
    twice = _keys(rng, 500)
    others = np.concatenate([common, _keys(rng, 15000), twice, twice])
    rng.shuffle(others)
    hs0 = np.empty(30000, dtype=np.uint64)
    hs0[0:16000:2] = heavy
    hs0[1:16000:2] = others[:8000]
    hs0[16000:] = others[8000:]
    hs1 = np.concatenate([common, [heavy], _keys(rng, 3000)]).astype(np.uint64)
    rng.shuffle(hs1)
    return [_asm(hs0), _asm(hs1)]


def _shared_fraction(frac, seed, n0=6000, n1=7000):
    """(e) `frac` of assembly 0's minimizers once in both assemblies"""
    rng = np.random.default_rng(seed)
    n_common = int(n0 * frac)
    common = _keys(rng, n_common)
    hs0 = np.concatenate([common, _keys(rng, n0 - n_common)])
    hs1 = np.concatenate([common, _keys(rng, n1 - n_common)])
    rng.shuffle(hs0)
    rng.shuffle(hs1)
    return [_asm(hs0), _asm(hs1)]


def _one_sided(seed):
    """(f) 40 000 minimizers of assembly 0 whose products all have bit 52 clear: all in coarse partition 0, whose sub-range for
    assembly 0 holds 20 000 + 5 000 + 4 096 -> 32 768 records.  The first attempt overflows it, the cursors say by how much, the
    second attempt has room (graph_join | 0x100)."""
    rng = np.random.default_rng(seed)
    prods = rng.integers(1, 2**63, size=40000, dtype=np.int64).astype(np.uint64) & np.uint64(ONES ^ (1 << 52))
    hs0 = _from_products(np.unique(prods))
    hs1 = np.concatenate([hs0[:9000], _keys(rng, 4000)])
    rng.shuffle(hs1)
    return [_asm(hs0), _asm(hs1)]


_CRAFTED, _CRAFTED_KEYS = _crafted(21)
CASES = {
    "crafted bits": _CRAFTED,
    "two assemblies": _thirds([3000, 2501], 22),
    "three assemblies": _thirds([2000, 1777, 2300], 23),
    "32 assemblies": _thirds([600 + 7 * a for a in range(32)], 24),
    "heavy key": _heavy(25),
}


def _one_attempt(lines, **want):
    assert len(lines) == 1, lines
    for key, val in want.items():
        assert lines[0][key] == val, (key, lines[0])


@pytest.mark.parametrize("name", list(CASES))
def test_12_byte_records_give_the_reference(name, monkeypatch, capfd):
    """(a), (b), (c): every case through the 12-byte records, and (d) through the 16-byte records of the shapes just beside them"""
    sets = CASES[name]
    ref = _reference(monkeypatch, capfd, name, sets)
    routes = [(R12, 12), (dict(R12, MXG_PJ_SKEW="1"), 12), ({"MXG_PJ_TWO_LEVEL": "1"}, 16), (dict(R12, MXG_PJ_PIPE="0"), 16),
              (dict(R12, MXG_PJ_REC12="0"), 16)]
    for env, nbytes in routes:
        states, joins, lines = _build(monkeypatch, capfd, sets, env)
        assert joins[0] == 2, (env, hex(joins[0]))
        _one_attempt(lines[0], pj=1, two_level=1, split=int("MXG_PJ_SPLIT" in env), record_bytes=nbytes, prefill0=0, P1=2)
        _check(states[0], ref, env)


def test_crafted_pairs_stay_apart(monkeypatch, capfd):
    """(a) said once more by name: the keys in both assemblies are vertices, their one-bit neighbours are not"""
    states, _, _ = _build(monkeypatch, capfd, _CRAFTED, R12)
    vh = states[0]["vertex_hash"]
    assert np.isin(_CRAFTED_KEYS["both"], vh).all()
    assert not np.isin(_CRAFTED_KEYS["only0"], vh).any() and not np.isin(_CRAFTED_KEYS["only1"], vh).any()


@pytest.mark.parametrize("frac,learnt", [(0.92, 1), (0.08, 0)], ids=["92 % shared", "8 % shared"])
@pytest.mark.parametrize("env", [R12, {"MXG_PJ_TWO_LEVEL": "1"}], ids=["12 bytes", "16 bytes"])
def test_second_build_uses_the_learnt_prefill(frac, learnt, env, monkeypatch, capfd):
    """(e) two builds on one handle: the first takes today's prefill, the second the learnt one where more than half of assembly 0
    was shared; both give the reference.  With MXG_PJ_PREFILL0=0 the second build keeps today's."""
    name = f"shared {frac}"
    sets = _shared_fraction(frac, 26)
    ref = _reference(monkeypatch, capfd, name, sets)
    shared0 = int((ref["flags"][0] == 7).sum())
    assert shared0 >= 0.9 * sets[0][0].size if learnt else shared0 <= 0.1 * sets[0][0].size
    states, joins, lines = _build(monkeypatch, capfd, sets, env, builds=3)
    for b in range(3):
        assert joins[b] == 2, hex(joins[b])
        _one_attempt(lines[b], two_level=1, prefill0=learnt if b else 0, record_bytes=12 if "MXG_PJ_SPLIT" in env else 16)
        _check(states[b], ref, (env, b))
    states, _, lines = _build(monkeypatch, capfd, sets, dict(env, MXG_PJ_PREFILL0="0"), builds=2)
    _one_attempt(lines[1], prefill0=0)
    _check(states[1], ref, "MXG_PJ_PREFILL0=0")


def test_learnt_prefill_with_runs_and_a_heavy_key(monkeypatch, capfd):
    """(c) + (e): followers, the skew path's references and duplicates of assembly 0 under the prefill "shared, own index".  The
    heavy-key pair of above with 21 000 of assembly 0's 30 000 minimizers shared, so that the second build learns the rule; a run
    of 70 equal hashes in sketch order (one leader per wave, followers without a record) lies over the tail."""
    rng = np.random.default_rng(27)
    heavy, run_key = _keys(rng, 2)
    common = _keys(rng, 21000)
    twice = _keys(rng, 300)
    others = np.concatenate([common, _keys(rng, 400), twice, twice])
    rng.shuffle(others)
    hs0 = np.empty(30000, dtype=np.uint64)
    hs0[0:16000:2] = heavy
    hs0[1:16000:2] = others[:8000]
    hs0[16000:] = others[8000:]
    hs0[29000:29070] = run_key
    hs1 = np.concatenate([common, [heavy, run_key], _keys(rng, 3000)]).astype(np.uint64)
    rng.shuffle(hs1)
    sets = [_asm(hs0), _asm(hs1)]
    ref = _reference(monkeypatch, capfd, "heavy learnt", sets)
    assert 2 * int((ref["flags"][0] == 7).sum()) > hs0.size
    for env in (R12, dict(R12, MXG_PJ_SKEW="1"), {"MXG_PJ_TWO_LEVEL": "1"}, dict(R12, MXG_PJ_PIPE="0")):
        states, joins, lines = _build(monkeypatch, capfd, sets, env, builds=2)
        _one_attempt(lines[1], prefill0=1)
        for b in range(2):
            _check(states[b], ref, (env, b))


def test_sub_range_overflow_converges(monkeypatch, capfd):
    """(f) a sub-range beyond its capacity: the first attempt reports it, the second is sized by the cursors and keeps 12 bytes;
    a second build on the handle starts with the learnt capacity (and, 9 000 of 40 000 shared, with today's prefill)"""
    sets = _one_sided(28)
    ref = _reference(monkeypatch, capfd, "one sided", sets)
    states, joins, lines = _build(monkeypatch, capfd, sets, R12, builds=2)
    assert joins[0] == 2 | 0x100, hex(joins[0])
    assert [ln["record_bytes"] for ln in lines[0]] == [12, 12] and lines[0][1]["rows2"] > lines[0][0]["rows2"]
    _check(states[0], ref, "first build")
    assert joins[1] == 2, hex(joins[1])
    _one_attempt(lines[1], record_bytes=12, prefill0=0)
    _check(states[1], ref, "second build")
