"""GPU test of the width of the graph stage's ordered passes (k_flags_pj, k_vertices_pj, k_adjacency, k_edge_flags, k_edges): a
thread block takes U = 1, 2 or 4 consecutive 256-blocks (MXG_GRAPH_U; by size otherwise: graph_tail_u in csrc/join_plan.h).
Every width, under every join, must leave the flags and the graph that U = 1 leaves; U = 1 under the default join is held
against the C oracle's graph stage (tests/_oracle.py) and the flags against numpy, so the comparison hangs on the reference and
not on the code under test.  Minimizer lists go straight to add_minimizers: no sketching, a few thousand entries at the most,
at the sizes where the indexing can go wrong (one more and one less than a 256-block, than a thread block of four)."""
import numpy as np
import pytest

from tests import _oracle

pytestmark = pytest.mark.gpu

WIDTHS = ("1", "2", "4")
JOINS = ({}, {"MXG_PJ_TWO_LEVEL": "1"}, {"MXG_GRAPH_JOIN": "global"})
KNOBS = ("MXG_GRAPH_U", "MXG_PJ_TWO_LEVEL", "MXG_GRAPH_JOIN")


def _keys(rng, n):
    """n distinct 64-bit keys"""
    out = np.unique(rng.integers(1, 2**63, size=n + 64, dtype=np.int64).astype(np.uint64))
    assert out.size >= n
    rng.shuffle(out)
    return out[:n]


def _records(n, borders):
    """record number per minimizer: a new record starts at every index in `borders`"""
    rec = np.zeros(n, np.uint32)
    for b in borders:
        if 0 < b < n:
            rec[b:] += 1
    return rec


def _assemblies(sizes, nv, seed, borders=None, shuffle=True):
    """len(sizes) assemblies; nv keys occur once in every one of them (the vertices), the others once in one assembly only"""
    rng = np.random.default_rng(seed)
    assert nv <= min(sizes)
    keys = _keys(rng, nv + sum(n - nv for n in sizes))
    shared, at, sets = keys[:nv], nv, []
    for a, n in enumerate(sizes):
        hs = np.concatenate([shared, keys[at:at + n - nv]])
        at += n - nv
        if shuffle:
            rng.shuffle(hs)
        bd = borders[a] if borders else sorted(rng.integers(1, max(n, 2), size=min(5, n)).tolist())
        rec = _records(n, bd)
        sets.append((hs, np.arange(n, dtype=np.uint32) * 3, rec, [f"c{i}" for i in range(int(rec.max()) + 1 if n else 1)]))
    return sets


def _with_runs(sets, a, runs):
    """assembly a: the minimizers [lo, hi) hold one key each run (a tandem array's run of equal hashes)"""
    hs = sets[a][0].copy()
    for lo, hi in runs:
        hs[lo:hi] = hs[lo]
    sets[a] = (hs,) + sets[a][1:]
    return sets


def _cases():
    c = {}
    # assembly sizes around one 256-block, a thread block of four, and three of those; three quarters of the smaller are vertices
    for n in (1, 255, 256, 257, 1023, 1024, 1025, 4 * 256 * 3 + 1):
        c[f"n{n}"] = _assemblies([n, n + 7], n - n // 4, seed=n)
    # the second assembly's only block shares a thread block with the first's tail; three assemblies ending inside thread blocks
    c["n300+5"] = _assemblies([300, 5], 4, seed=2)
    c["n1+257+1025"] = _assemblies([1, 257, 1025], 1, seed=3)
    # vertex counts (= positions of the adjacency and edge passes) around the same borders; 0: no key in common
    for nv in (0, 1, 255, 256, 257, 1025):
        c[f"nv{nv}"] = _assemblies([nv + 300, nv + 77], nv, seed=100 + nv)
    # every minimizer a vertex, in the same order in both assemblies: filtered position = index.  Record borders at a sub-block
    # border (256, 768), at the border of a thread block of two (512) and of four (1024), and one off: no edge may cross them
    c["record borders"] = _assemblies([1300, 1300], 1300, seed=5, shuffle=False,
                                      borders=[[256, 512, 768, 1024], [255, 257, 511, 1023, 1025]])
    # runs of equal hashes across the same borders: a follower on lane 0 of a sub-block, its leader on lane 63 of the one before
    c["runs across borders"] = _with_runs(_assemblies([1300, 1290], 900, seed=6), 0,
                                          [(254, 258), (511, 514), (767, 769), (1023, 1025), (1279, 1300)])
    c["A5"] = _assemblies([300, 411, 257, 520, 333], 200, seed=7)   # more than four assemblies: k_edge_flags looks the masks up
    c["A9"] = _assemblies([300 + 17 * a for a in range(9)], 190, seed=8)  # more than eight: k_edges does
    return c


CASES = _cases()
_REFERENCE = {}


def _reference(name):
    """flags from numpy, vertices and edges from the C oracle: once per case"""
    if name not in _REFERENCE:
        sets = CASES[name]
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
        g = _oracle.load().graph([s[0] for s in sets], [s[2] for s in sets], [1.0 + a / 4 for a in range(len(sets))], edges=True)
        edges = sorted(zip(g["eu"].tolist(), g["ev"].tolist(), g["esup"].tolist(), g["ew"].tolist()))
        _REFERENCE[name] = {"flags": flags, "vertices": g["vertices"], "unique": g["unique"], "edges": edges}
    return _REFERENCE[name]


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
        eng.build_graph()  # twice on one handle: the counts of the passes must come back clean
        return _state(eng, len(sets))


@pytest.mark.parametrize("name", list(CASES))
def test_every_width_under_every_join_equals_width_one(name, monkeypatch):
    sets = CASES[name]
    base = _build(monkeypatch, sets, {"MXG_GRAPH_U": "1"})
    # width 1, default join, against the reference
    ref = _reference(name)
    for a in range(len(sets)):
        assert np.array_equal(base[f"flags{a}"], ref["flags"][a]), f"flags of assembly {a}"
    assert sum(int((base[f"flags{a}"] & 1).sum()) for a in range(len(sets))) == ref["unique"]
    assert len(base["vertex_hash"]) == ref["vertices"]
    vh = base["vertex_hash"]
    got = sorted(zip(vh[base["edge_u"]].tolist(), vh[base["edge_v"]].tolist(), base["edge_support"].tolist(), base["edge_weight"].tolist()))
    assert got == ref["edges"]
    for a, s in enumerate(sets):  # every vertex sits where its key does in every assembly
        where = {int(h): i for i, h in enumerate(s[0].tolist())}
        idx = np.array([where[int(h)] for h in vh.tolist()], dtype=np.int64)
        assert np.array_equal(base["vertex_pos"][a], s[1][idx]) and np.array_equal(base["vertex_record"][a], s[2][idx]), a
    # every other width and join against it
    for join in JOINS:
        for u in WIDTHS:
            if u == "1" and not join:
                continue
            other = _build(monkeypatch, sets, dict(join, MXG_GRAPH_U=u))
            assert other.keys() == base.keys()
            for key in base:
                assert np.array_equal(base[key], other[key]), (key, u, join)


def test_default_width_is_by_size_and_equals_width_one(monkeypatch):
    """no knob: the size rule picks the width (1 at this size); an unknown value of the knob is no width"""
    sets = CASES["n1025"]
    base = _build(monkeypatch, sets, {"MXG_GRAPH_U": "1"})
    for env in ({}, {"MXG_GRAPH_U": "3"}, {"MXG_GRAPH_U": "0"}):
        other = _build(monkeypatch, sets, env)
        for key in base:
            assert np.array_equal(base[key], other[key]), (key, env)


def test_fused_call_at_width_four_equals_two_calls_at_width_one(monkeypatch):
    """sketch_graph() (the counts still on the device, the join partitioned under the sketches) at U = 4 against sketch() +
    build_graph() at U = 1, on a 2 x 2 Mbp synthetic pair"""
    import torch
    from ntjoin_amd import synth
    from ntjoin_amd.engine import MxEngine
    ref, tgt = synth.config2(seed=7, n_bases=2_000_000)

    def run(fused, env):
        for key in KNOBS:
            monkeypatch.delenv(key, raising=False)
        for key, val in env.items():
            monkeypatch.setenv(key, val)
        with MxEngine(k=32, w=1000) as eng:
            for name, wt, recs in (("ref", 2.0, ref), ("tgt", 1.0, tgt)):
                words, starts, lens = synth.pack_records(recs)
                d = torch.from_numpy(words.view(np.int32)).cuda()
                eng.add_packed_device(name, wt, d.data_ptr(), starts, lens, keepalive=d)
            if fused:
                eng.sketch_graph()
            else:
                eng.sketch()
                eng.build_graph()
            return _state(eng, 2)

    want = run(False, {"MXG_GRAPH_U": "1"})
    assert len(want["vertex_hash"]) > 1000 and len(want["edge_u"]) > 1000
    got = run(True, {"MXG_GRAPH_U": "4"})
    assert got.keys() == want.keys()
    for key in want:
        assert np.array_equal(want[key], got[key]), key
