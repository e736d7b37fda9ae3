"""GPU test of level 1 of the two-level join (k_pj1_scatter) at G = 1 and 2 tiles of 4096 minimizers per thread block
(MXG_PJ_TILES forces G on the 12-byte route; join_plan.h's pj1_tiles chooses it otherwise, and keeps the 16-byte route at 1).
Minimizer lists go in through add_minimizers; MXG_PJ_TWO_LEVEL=1 forces two levels at these sizes (P1 = 2 coarse partitions),
MXG_PJ_SPLIT=1 gives every assembly its own sub-ranges and launches (the fused call's layout, 12-byte records); without it one
launch covers all assemblies (one cursor per coarse partition, 16-byte records, one tile per block whatever is forced).  Every
build must give the flags numpy gives, the vertices and edges of the C oracle and the state of the global-table join, and its
MXG_DEBUG_JOIN line must name the G that ran.

The shapes are the smallest at which a block of G tiles can go wrong: sizes around a tile (4096) and a group (G x 4096), a small
assembly between large ones, borders of assemblies inside a tile, runs of equal hashes across a tile's and a group's border, a
key of high multiplicity, a sub-range that overflows, the learnt prefill and both record sizes.

Widths of four tiles, and of two and four at level 2, were measured slower at every size and are not built
(profiles/r13/join_tiles_ab.txt), so nothing here forces them."""
import numpy as np
import pytest

from tests.test_gpu_join_records import R12, _build as _records_build, _heavy, _one_sided, _reference, _shared_fraction
from tests.test_gpu_join_verdicts import _asm, _check, _keys

pytestmark = pytest.mark.gpu

TILE = 4096
WIDTHS = (1, 2)
ONE_CURSOR = {"MXG_PJ_TWO_LEVEL": "1"}


def _build(monkeypatch, capfd, sets, env, g, builds=1):
    monkeypatch.delenv("MXG_PJ_TILES", raising=False)
    return _records_build(monkeypatch, capfd, sets, dict(env, MXG_PJ_TILES=str(g)), builds=builds)


def _ran_at(lines, g, **want):
    """every attempt of a build ran level 1 at G = g"""
    assert lines, "no [mxg] join line"
    for ln in lines:
        assert ln["two_level"] == 1 and ln["tiles1"] == g, ln
        for key, val in want.items():
            assert ln[key] == val, (key, ln)


def _mixed(sizes, seed):
    """assemblies of exactly these sizes: a third of the smallest (at least its one minimizer) in every assembly, some keys twice
    in their own, the rest their own"""
    rng = np.random.default_rng(seed)
    n_common = max(min(sizes) // 3, 1)
    common = _keys(rng, n_common)
    sets = []
    for n in sizes:
        twice = _keys(rng, (n - n_common) // 8)
        hs = np.concatenate([common, _keys(rng, n - n_common - 2 * twice.size), twice, twice])
        assert hs.size == n
        rng.shuffle(hs)
        sets.append(_asm(hs))
    return sets


# around one tile, one group of two tiles and two groups
SIZES = sorted({1} | {m * TILE + d for m in (1, 2, 4) for d in (-1, 0, 1)})


@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_a_tile_and_a_group(n, monkeypatch, capfd):
    """an assembly of n minimizers beside one of 3000, with sub-ranges (its own launches: ceil(n / 4096) tiles, a ragged last
    group where that is odd) and on the one-cursor layout (the border of the assemblies at n, inside a tile unless n is a
    multiple of 256; G stays 1 there)"""
    sets = _mixed([n, 3000], 100 + n)
    ref = _reference(monkeypatch, capfd, f"tiles: size {n}", sets)
    for g in WIDTHS:
        for env, nbytes, ran in ((R12, 12, g), (ONE_CURSOR, 16, 1)):
            states, joins, lines = _build(monkeypatch, capfd, sets, env, g)
            assert joins[0] == 2, (env, g, hex(joins[0]))
            _ran_at(lines[0], ran, record_bytes=nbytes, split=int(env is R12))
            _check(states[0], ref, (env, g))


BORDERS = {
    # 256-blocks 0..19 | 20..47: the border lies in tile 1 (blocks 16..31)
    "border inside a tile": ([5000, 7000], ONE_CURSOR),
    # three assemblies, the middle one smaller than a tile: on the one-cursor layout both its borders lie in tile 2; with
    # sub-ranges its launch is one tile, a ragged group, beside launches of three and two tiles
    "small middle assembly": ([9000, 300, 6000], ONE_CURSOR),
    "small middle assembly, sub-ranges": ([9000, 300, 6000], R12),
}


@pytest.mark.parametrize("name", list(BORDERS))
def test_assembly_borders_and_a_small_assembly(name, monkeypatch, capfd):
    sizes, env = BORDERS[name]
    sets = _mixed(sizes, 7 + len(name))
    ref = _reference(monkeypatch, capfd, "tiles: " + name, sets)
    for g in WIDTHS:
        states, joins, lines = _build(monkeypatch, capfd, sets, env, g)
        assert joins[0] == 2, (g, hex(joins[0]))
        _ran_at(lines[0], g if env is R12 else 1, split=int(env is R12))
        _check(states[0], ref, (name, g))


def _runs_over_borders(seed):
    """runs of equal hashes in assembly 0 (20 000 minimizers) across the tile border at 4096 (inside a group of two), the group
    borders at 8192 and 16 384, one that ends exactly at a border and one that starts there; every second run's key lies once
    in assembly 1"""
    rng = np.random.default_rng(seed)
    common = _keys(rng, 5000)
    hs0 = np.concatenate([common, _keys(rng, 15000)])
    rng.shuffle(hs0)
    spans = [(4090, 4101), (8185, 8200), (16380, 16390), (12280, 12288), (12288, 12300), (8000, 8192 + 70)]
    # (the last: 262 equal hashes over five waves and the group border; it covers the second span)
    run_keys = _keys(rng, len(spans))
    for key, (lo, hi) in zip(run_keys, spans):
        hs0[lo:hi] = key
    hs1 = np.concatenate([np.unique(common), run_keys[::2], _keys(rng, 2500)])
    rng.shuffle(hs1)
    return [_asm(hs0), _asm(hs1)]


def test_runs_across_tile_and_group_borders(monkeypatch, capfd):
    sets = _runs_over_borders(31)
    ref = _reference(monkeypatch, capfd, "tiles: runs", sets)
    assert (ref["flags"][0] == 4).sum() >= 20  # followers and leaders of runs whose key is in every assembly
    for g in WIDTHS:
        for env in (R12, ONE_CURSOR):
            states, joins, lines = _build(monkeypatch, capfd, sets, env, g)
            assert joins[0] == 2, (env, g, hex(joins[0]))
            _ran_at(lines[0], g if env is R12 else 1)
            _check(states[0], ref, (env, g))


def test_heavy_key_behind_blocks_of_two_tiles(monkeypatch, capfd):
    """test_gpu_join_records' heavy key (8 000 copies in assembly 0, never neighbours): one coarse bin of a block takes a third of
    its records, and level 2's skew path collapses them behind it, by itself and with MXG_PJ_SKEW=1 in every partition"""
    sets = _heavy(25)
    ref = _reference(monkeypatch, capfd, "tiles: heavy key", sets)
    for g in WIDTHS:
        for env in (R12, dict(R12, MXG_PJ_SKEW="1")):
            states, joins, lines = _build(monkeypatch, capfd, sets, env, g)
            assert joins[0] == 2, (env, g, hex(joins[0]))
            _ran_at(lines[0], g, record_bytes=12)
            _check(states[0], ref, (env, g))


def test_sub_range_overflow_converges_at_every_width(monkeypatch, capfd):
    """test_gpu_join_records' one-sided assembly: the first attempt overflows a sub-range (records past `cap` are dropped by the
    rule pos >= cap, whichever tile of the block they came from), the cursors say by how much, the second has room; a second
    build starts with the learnt capacity"""
    sets = _one_sided(28)
    ref = _reference(monkeypatch, capfd, "tiles: one sided", sets)
    for g in WIDTHS:
        states, joins, lines = _build(monkeypatch, capfd, sets, R12, g, builds=2)
        assert joins[0] == 2 | 0x100 and joins[1] == 2, (g, hex(joins[0]), hex(joins[1]))
        assert len(lines[0]) == 2 and lines[0][1]["rows2"] > lines[0][0]["rows2"] and len(lines[1]) == 1, (g, lines)
        for b in range(2):
            _ran_at(lines[b], g, record_bytes=12)
            _check(states[b], ref, (g, b))


def test_learnt_prefill_and_both_record_sizes(monkeypatch, capfd):
    """two builds of equal sizes, 92 % of assembly 0 shared: the second takes the learnt prefill; 12-byte records at G = 2 against
    16-byte records, which keep G = 1"""
    sets = _shared_fraction(0.92, 26, n0=9000, n1=10000)
    ref = _reference(monkeypatch, capfd, "tiles: shared 0.92", sets)
    for env, nbytes, ran in ((R12, 12, 2), (dict(R12, MXG_PJ_REC12="0"), 16, 1), (ONE_CURSOR, 16, 1)):
        states, joins, lines = _build(monkeypatch, capfd, sets, env, 2, builds=2)
        for b in range(2):
            assert joins[b] == 2, (env, hex(joins[b]))
            _ran_at(lines[b], ran, record_bytes=nbytes, prefill0=b)
            _check(states[b], ref, (env, b))


def test_width_by_size_when_nothing_is_forced(monkeypatch, capfd):
    """no MXG_PJ_TILES: launches of these sizes (a handful of tiles, far below the threshold) run at G = 1"""
    sets = _mixed([9000, 300, 6000], 51)
    ref = _reference(monkeypatch, capfd, "tiles: by size", sets)
    monkeypatch.delenv("MXG_PJ_TILES", raising=False)
    states, joins, lines = _records_build(monkeypatch, capfd, sets, R12)
    assert joins[0] == 2, hex(joins[0])
    _ran_at(lines[0], 1, record_bytes=12)
    _check(states[0], ref, "by size")
