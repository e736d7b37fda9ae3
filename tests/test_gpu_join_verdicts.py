"""GPU test of the partitioned join's verdict words (ntjoin_amd/csrc/join_verdict.h) and of where its records lie: the
partitioning kernels prefill every minimizer's verdict with "once in its assembly, not in every assembly", the join kernels send
only the verdicts that differ, and a record of the pipelined join kernel finds its segment through a per-record region number.
Minimizer lists go in through add_minimizers (nothing is sketched); every case runs on the one-level route, the two-level route with the pipelined and the plain join kernel and with the
second level's skew path, and must give the flags numpy gives, the vertices and edges of the C oracle, and the state of the
global-table join.  Each case names the kinds of verdict it is about and is refused if its reference lacks one of them."""
import numpy as np
import pytest

from tests import _oracle

pytestmark = pytest.mark.gpu

KNOBS = ("MXG_GRAPH_JOIN", "MXG_PJ_TWO_LEVEL", "MXG_PJ_PIPE", "MXG_PJ_SKEW", "MXG_PJ_FORCE_FAIL", "MXG_PJ_EARLY")
ROUTES = [{}, {"MXG_PJ_TWO_LEVEL": "1"}, {"MXG_PJ_TWO_LEVEL": "1", "MXG_PJ_PIPE": "0"}, {"MXG_PJ_TWO_LEVEL": "1", "MXG_PJ_SKEW": "1"}]
FAILS = [{"MXG_PJ_FORCE_FAIL": "1"}, {"MXG_PJ_TWO_LEVEL": "1", "MXG_PJ_FORCE_FAIL": "1"}]
MUL = 0x9E3779B97F4A7C15
INV = pow(MUL, -1, 1 << 64)
ONES = (1 << 64) - 1

# the join's multiplier: partition and slot are bit fields of key * MUL, the special keys are chosen by their products
# verdict kinds by flag byte (MXG_MX_UNIQUE 1, MXG_MX_SHARED 2, MXG_MX_INALL 4)
SKIPPED = 1       # once in its assembly, not in every assembly: the prefill, never sent by the join
SHARED = 7        # once in every assembly: a vertex
ONCE_HERE = 5     # once in its assembly, in every assembly, more than once in another
DUP = 0           # more than once in its assembly, not in every assembly
DUP_INALL = 4     # more than once in its assembly, in every assembly


def _keys(rng, n):
    return rng.integers(1, 2**63, size=n, dtype=np.int64).astype(np.uint64)


def _asm(hs, n_rec=7):
    hs = np.ascontiguousarray(hs, dtype=np.uint64)
    rec = (np.arange(hs.size, dtype=np.uint64) * n_rec // max(hs.size, 1)).astype(np.uint32)
    return hs, np.arange(hs.size, dtype=np.uint32) * 3, rec, [f"c{i}" for i in range(n_rec)]


def _thirds(sizes, seed):
    """a third of the smaller assembly's keys in every assembly, a third only in their own, a third twice in their own"""
    rng = np.random.default_rng(seed)
    third = min(sizes) // 3
    common = _keys(rng, third)
    sets = []
    for n in sizes:
        twice = _keys(rng, third // 2)
        own = _keys(rng, n - third - 2 * twice.size)
        hs = np.concatenate([common, own, twice, twice])
        rng.shuffle(hs)
        sets.append(_asm(hs))
    return sets


def _two_of_three(seed):
    """keys in exactly two of three assemblies (once in each: skipped in both), beside keys in all three and in one"""
    rng = np.random.default_rng(seed)
    common, ab, ac, bc = _keys(rng, 400), _keys(rng, 300), _keys(rng, 300), _keys(rng, 300)
    sets = []
    for parts, n_own in (((common, ab, ac), 211), ((common, ab, bc), 97), ((common, ac, bc), 333)):
        hs = np.concatenate(list(parts) + [_keys(rng, n_own)])
        rng.shuffle(hs)
        sets.append(_asm(hs))
    return sets


def _runs(seed):
    """runs of equal hashes of length 2, 64, 65 and 200 that start at lanes 0, 62 and 63 of a wave, the wave being the last of
    its 256-block (lanes 62 and 63: leader and followers in different waves AND 256-blocks; lane 0 with 65 or 200: likewise).
    The run keys alternate between "once in the two other assemblies" and "nowhere else"; the last run's key lies once in
    assembly 1 and not in assembly 2, where its one minimizer keeps the prefill."""
    rng = np.random.default_rng(seed)
    combos = [(ln, lane) for ln in (2, 64, 65, 200) for lane in (0, 62, 63)]
    n0 = 512 * (len(combos) + 1)
    common = _keys(rng, 1500)
    run_keys = _keys(rng, len(combos))
    hs0 = np.concatenate([common, _keys(rng, n0 - common.size)])
    rng.shuffle(hs0)
    for j, (ln, lane) in enumerate(combos):
        start = 512 * (j + 1) - 64 + lane
        hs0[start:start + ln] = run_keys[j]
    elsewhere = run_keys[0:len(combos) - 1:2]
    hs1 = np.concatenate([np.unique(common), elsewhere, run_keys[-1:], _keys(rng, 700)])
    hs2 = np.concatenate([np.unique(common), elsewhere, _keys(rng, 433)])
    rng.shuffle(hs1)
    rng.shuffle(hs2)
    return [_asm(hs0), _asm(hs1), _asm(hs2)]


def _alone(seed):
    """one assembly: every key that occurs once is shared, nothing keeps the prefill"""
    rng = np.random.default_rng(seed)
    twice = _keys(rng, 300)
    hs = np.concatenate([_keys(rng, 2000), twice, twice])
    rng.shuffle(hs)
    return [_asm(hs)]


def _special(seed):
    """key 0, the all-ones key, the key whose product is the table's empty mark and two keys whose products agree in bits 32..63
    (same partition, same first slot), once in each assembly"""
    rng = np.random.default_rng(seed)
    hi = 0x5A17C3E9 << 32
    special = np.array([0, ONES, (ONES * INV) & ONES, ((hi | 1) * INV) & ONES, ((hi | 2) * INV) & ONES], dtype=np.uint64)
    assert (int(special[2]) * MUL) & ONES == ONES
    assert ((int(special[3]) * MUL) & ONES) >> 32 == ((int(special[4]) * MUL) & ONES) >> 32
    common = _keys(rng, 500)
    sets = []
    for n_own in (389, 277):
        twice = _keys(rng, 50)
        hs = np.concatenate([special, common, _keys(rng, n_own), twice, twice])
        rng.shuffle(hs)
        sets.append(_asm(hs))
    return sets, special


def _heavy(seed):
    """one key 5 000 times in assembly 0, never twice in a row, and once in assembly 1, among 20 000 other keys: its partition
    holds more than 1 024 records, so the join kernels walk it with the loop behind the first four records per thread"""
    rng = np.random.default_rng(seed)
    common = _keys(rng, 6000)
    heavy = _keys(rng, 1)[0]
    others = np.concatenate([common, _keys(rng, 14000)])
    rng.shuffle(others)
    hs0 = np.empty(25000, dtype=np.uint64)
    hs0[0:10000:2] = heavy
    hs0[1:10000:2] = others[:5000]
    hs0[10000:] = others[5000:]
    hs1 = np.concatenate([common, [heavy], _keys(rng, 3000)]).astype(np.uint64)
    rng.shuffle(hs1)
    return [_asm(hs0), _asm(hs1)]


_SPECIAL, _SPECIAL_KEYS = _special(15)
CASES = {
    "thirds 3000+2500": (_thirds([3000, 2500], 11), (SKIPPED, SHARED, DUP)),
    "two of three": (_two_of_three(12), (SKIPPED, SHARED)),
    "runs": (_runs(13), (SKIPPED, SHARED, DUP, DUP_INALL, ONCE_HERE)),
    "one assembly": (_alone(14), (SHARED, DUP_INALL)),
    "special keys": (_SPECIAL, (SKIPPED, SHARED, DUP)),
    "heavy key": (_heavy(16), (SKIPPED, SHARED, DUP_INALL, ONCE_HERE)),
}
_REFERENCE = {}


def _truth(sets):
    allk = np.concatenate([s[0] for s in sets])
    uniq, inv = np.unique(allk, return_inverse=True)
    cnt = np.zeros((len(sets), uniq.size), np.int64)
    at = 0
    for a, s in enumerate(sets):
        np.add.at(cnt[a], inv[at:at + s[0].size], 1)
        at += s[0].size
    inall, once = (cnt > 0).all(axis=0), (cnt == 1).all(axis=0)
    flags, at = [], 0
    for a, s in enumerate(sets):
        k = inv[at:at + s[0].size]
        at += s[0].size
        flags.append(((cnt[a][k] == 1) * 1 | once[k] * 2 | inall[k] * 4).astype(np.uint8))
    return flags


def _state(eng, n_asm):
    out = {f"flags{a}": eng.get_mx_flags(a).copy() for a in range(n_asm)}
    for key, val in eng.get_graph().items():
        out[key] = np.asarray(val).copy()
    return out


def _build(monkeypatch, sets, env):
    from ntjoin_amd.engine import MxEngine
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    with MxEngine(k=32, w=1000) as eng:
        for a, (hs, pos, rec, ids) in enumerate(sets):
            eng.add_minimizers(f"a{a}", 1.0 + a / 4, hs, pos, rec, ids)
        eng.build_graph()
        return _state(eng, len(sets)), int(eng.stats()["graph_join"])


def _reference(monkeypatch, name):
    """flags from numpy, vertices and edges from the C oracle, the state of the global-table join: once per case"""
    if name not in _REFERENCE:
        sets, kinds = CASES[name]
        flags = _truth(sets)
        allf = np.concatenate(flags)
        for kind in kinds:  # a case cannot pass empty
            assert (allf == kind).any(), f"case '{name}' has no verdict of kind {kind}"
        g = _oracle.load().graph([s[0] for s in sets], [s[2] for s in sets], [1.0 + a / 4 for a in range(len(sets))], edges=True)
        edges = sorted(zip(g["eu"].tolist(), g["ev"].tolist(), g["esup"].tolist(), g["ew"].tolist()))
        state, join = _build(monkeypatch, sets, {"MXG_GRAPH_JOIN": "global"})
        assert join & 0xFF == 3, hex(join)
        _REFERENCE[name] = {"flags": flags, "vertices": g["vertices"], "edges": edges, "global": state}
    return _REFERENCE[name]


def _check(got, ref, what):
    for a, fl in enumerate(ref["flags"]):
        assert np.array_equal(got[f"flags{a}"], fl), (what, f"flags of assembly {a}")
    vh = got["vertex_hash"]
    assert len(vh) == ref["vertices"], what
    edges = sorted(zip(vh[got["edge_u"]].tolist(), vh[got["edge_v"]].tolist(), got["edge_support"].tolist(), got["edge_weight"].tolist()))
    assert edges == ref["edges"], what
    assert got.keys() == ref["global"].keys(), what
    for key in got:
        assert np.array_equal(got[key], ref["global"][key]), (what, key)


@pytest.mark.parametrize("name", list(CASES))
def test_every_route_gives_the_reference_verdicts(name, monkeypatch):
    ref = _reference(monkeypatch, name)
    _check(ref["global"], ref, "global table")
    for env in ROUTES:
        got, join = _build(monkeypatch, CASES[name][0], env)
        assert join & 0xFF == (2 if "MXG_PJ_TWO_LEVEL" in env else 1), (env, hex(join))
        _check(got, ref, env)


def test_special_keys_are_vertices(monkeypatch):
    """the five special keys occur once in each assembly: all of them are vertices on every route"""
    for env in ROUTES:
        got, _ = _build(monkeypatch, _SPECIAL, env)
        assert np.isin(_SPECIAL_KEYS, got["vertex_hash"]).all(), env


@pytest.mark.parametrize("env", FAILS, ids=["one level", "two levels"])
def test_redo_with_the_global_table_does_not_see_the_prefill(env, monkeypatch):
    name = "thirds 3000+2500"
    ref = _reference(monkeypatch, name)
    got, join = _build(monkeypatch, CASES[name][0], env)
    assert join & 0xFF == 3, hex(join)  # the LDS join reported failure: the stage ran again with the global table
    _check(got, ref, env)


@pytest.mark.parametrize("w", [50, 200])
def test_fused_call_prefills_and_skips(w, monkeypatch):
    """mxg_sketch_graph on real sketches of a 2 Mbp synthetic pair, against MXG_PJ_EARLY=0 and the global table.  At w = 200 every
    assembly is partitioned (and prefilled) behind its own sketch, one sub-range per assembly (graph_join | 0x400).  At w = 50 the
    sketches of this pair do not go through the streams as one batch each, so the call partitions behind the last sketch (no
    0x400): the case pins the fused call's own sizes-on-the-device route through k_pj1_scatter's prefill."""
    import torch
    from ntjoin_amd import synth
    from ntjoin_amd.engine import MxEngine
    ref, tgt = synth.config2(seed=3, n_bases=2_000_000)

    def run(env):
        for key in KNOBS:
            monkeypatch.delenv(key, raising=False)
        for key, val in env.items():
            monkeypatch.setenv(key, val)
        with MxEngine(k=32, w=w) as eng:
            for name, wt, recs in (("ref", 2.0, ref), ("tgt", 1.0, tgt)):
                words, starts, lens = synth.pack_records(recs)
                d = torch.from_numpy(words.view(np.int32)).cuda()
                eng.add_packed_device(name, wt, d.data_ptr(), starts, lens, keepalive=d)
            eng.sketch_graph()
            hashes = [np.array(eng.get_sketch(a)["out_hash"], copy=True) for a in range(2)]
            return _state(eng, 2), int(eng.stats()["graph_join"]), hashes

    early, join, hashes = run({"MXG_PJ_TWO_LEVEL": "1"})
    assert join == (2 | 0x400 if w == 200 else 2), hex(join)
    truth = _truth([(h,) for h in hashes])
    allf = np.concatenate(truth)
    for kind in (SKIPPED, SHARED):  # the verdict the join leaves to the prefill, and one it sends
        assert (allf == kind).any(), f"no verdict of kind {kind}"
    for a in range(2):
        assert np.array_equal(early[f"flags{a}"], truth[a]), a
    for env in ({"MXG_PJ_TWO_LEVEL": "1", "MXG_PJ_EARLY": "0"}, {"MXG_GRAPH_JOIN": "global"}):
        other, jo, _ = run(env)
        assert not jo & 0x400, hex(jo)
        assert other.keys() == early.keys()
        for key in early:
            assert np.array_equal(early[key], other[key]), (env, key)
