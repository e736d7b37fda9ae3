"""GPU tests of mxg_synteny_assess (include/ntjoin_mx.h, row f13) against the sequential restatement of the contract
(tests/_assess_restatement.py) applied to the blocks mxg_synteny_blocks returned: the hand-made cases of tests/_assess_cases.py, block
counts around the wave, the 256-thread block, the 1024-element tile of the scans and of the sort and past 2^16, one chain over all
blocks and a chain per block, subject keys sorted, reversed, equal, interleaved and under one long interval -- at the head of the
order, on the last place of a tile and on the last place of the first round of the running maximum --, piece tables, each parameter
at 0, three assemblies, every refusal with the handle usable afterwards, and the PAF text after an assess call."""
import ctypes as C
import time

import numpy as np
import pytest

from tests import _assess_cases as AC, _assess_restatement as A, _cover_scale as CS, _synteny_cases as cases, _synteny_restatement as R
from tests.test_gpu_synteny import as_tuples, device, load

pytestmark = pytest.mark.gpu

ANCHOR = AC.anchor_cases()
SCALARS = ("n_blocks", "n_chains", "n_breakpoints", "query_bases", "subject_bases", "aligned_query", "chained_subject", "covered_subject",
           "breakpoints", "na", "nga", "ng")
A_FWD, A_REV, A_GAP = 0, 1, 2


def check(eng, case, assess=None, **over):
    "one blocks call, one assess call; the restatement over the blocks that came back -> (blocks result, restated assessment)"
    c = dict(case, **over)
    blocks = device(eng, c)
    params = dict(c.get("assess", {}) if assess is None else assess)
    got = eng.synteny_assess(**params)
    want = A.assess(as_tuples(blocks), c["k"], R.query_lengths(c["lengths"][c["q"]], c["pieces"], c["first"]), c["lengths"][c["s"]],
                    pieces=c["pieces"], first=c["first"], **params)
    for key in SCALARS:
        assert got[key] == want[key], (key, got[key], want[key])
    for name in A.CHAIN_FIELDS:
        assert got["chains"][name].tolist() == want["chains"][name], name
    for name in A.BP_FIELDS:
        assert got["bps"][name].tolist() == want["bps"][name], name
    return blocks, want


@pytest.mark.parametrize("name", sorted(ANCHOR))
def test_hand_cases(name):
    case, expect = ANCHOR[name]
    with load(case) as eng:
        blocks, want = check(eng, case)
    assert blocks["n_blocks"] == case["n_specs"] and AC.matches(want, expect)


def test_subject_of_no_bases():
    """D == 0 on the device: the blocks call takes subject_length = [0] as given (it reads the lengths only for the PAF text), so
    subject_bases is 0 and nga and ng are zeros while na is not"""
    case, _ = ANCHOR["nx"]
    with load(case) as eng:
        _, want = check(eng, case, lengths=[[0], case["lengths"][1]])
    zeros = dict(n50=0, l50=0, n75=0, l75=0, n90=0, l90=0)
    assert want["subject_bases"] == 0 and want["nga"] == zeros and want["ng"] == zeros and want["na"]["n50"] == 132


@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 65537])
def test_block_counts(n):
    "a seeded mix of joins, jumps, turns and record borders; then with merge_gap below every gap (118): a chain per block"
    case = AC.row_case(n, "mixed", seed=n + 1)
    with load(case) as eng:
        blocks, want = check(eng, case)
        assert blocks["n_blocks"] == n
        if n > 2:
            assert 1 < want["n_chains"] < n and want["n_breakpoints"] > 0
        if n <= 1025:
            check(eng, case, assess=dict(merge_gap=100))


def test_one_chain_of_4097_blocks_and_4097_chains_of_one():
    case = AC.row_case(4097, "chain")
    with load(case) as eng:
        blocks, want = check(eng, case)
        assert blocks["n_blocks"] == 4097 and want["n_chains"] == 1 and want["chains"]["n_anchors"] == [2 * 4097] and want["n_breakpoints"] == 0
        _, want = check(eng, case, assess=dict(merge_gap=100))   # (the gaps are 118)
        assert want["n_chains"] == 4097 and want["breakpoints"][(A.RELOCATION, 0)] == 4096
        assert want["covered_subject"] == want["chained_subject"] == 4097 * 82


@pytest.mark.parametrize("mode", ["apart", "reversed", "interleaved"])
def test_subject_orders(mode):
    "chains whose subject keys are already sorted, reversed, and dealt to two subject records in turn; disjoint: covered = chained"
    case = AC.row_case(2500, mode)
    with load(case) as eng:
        blocks, want = check(eng, case)
    assert blocks["n_blocks"] == want["n_chains"] == 2500 and want["covered_subject"] == want["chained_subject"] == 2500 * 82


def test_equal_subject_keys():
    """the query's one chain seen through 1300 table records that are prefixes of different lengths of it: every chain starts at the
    same subject place and ends elsewhere, so all sort keys are equal and the union is the longest one.  This is no test of the
    sort's stability: the union is the same in whatever order chains of one whole key come out, and nothing reads that order today.
    What pins the stability of the single passes here is every result that takes more than one pass (the other tests of this file);
    the direct test of the sort's stability is tests/test_gpu_primitives.py::test_sort (values = indices against numpy's stable argsort)"""
    case = AC.row_case(40, "chain")
    ln = case["lengths"][1][0]
    ends = [min(ln, 250 + 200 * (r * 7 % 39)) for r in range(1300)]
    with load(case) as eng:
        _, want = check(eng, case, pieces=[(0, 0, e, A_FWD) for e in ends], first=list(range(len(ends) + 1)))
    assert want["n_chains"] == 1300 and len(set(want["chains"]["s_start"])) == 1 and len(set(want["chains"]["s_end"])) > 30
    assert want["covered_subject"] == max(want["chains"]["s_end"]) - want["chains"]["s_start"][0] < want["chained_subject"]


def test_one_long_interval_covers_every_later_one():
    "2900 chains inside the first: across the tile borders of the sort and of the max scan the running maximum stays the first one's"
    case = AC.cover_case(2900)
    with load(case) as eng:
        blocks, want = check(eng, case)
    assert blocks["n_blocks"] == 2960 and want["n_chains"] == 2901
    assert want["covered_subject"] == want["chains"]["s_end"][0] - want["chains"]["s_start"][0] == 60 * 200 - 118


@pytest.mark.parametrize("m0,m1", CS.CARRY_CASES)
def test_chains_under_a_long_chain_behind_a_carry(m0, m1):
    """tests/_cover_scale.py: two subject records, on each one long chain over m single ones.  Sorted by subject place the second
    record's long chain stands on place m0 + 1 -- the last of tile 0, and the last of the first round of k_pt_max_tiles (256 tiles) --
    and its singles behind the border: the largest subject end in front of them is the carry, and it must be their own record's chain.
    tests/test_maxscan_model_cpu.py shows that covered_subject differs when that carry is dropped or comes a tile early"""
    from ntjoin_amd.engine import MxEngine
    t0 = time.time()
    case = CS.cover_scale_case(m0, m1)
    with MxEngine(k=case["k"], w=10) as eng:
        for a, asm in enumerate(case["asms"]):
            eng.add_minimizers(f"asm{a}", 1.0, asm["hash"], asm["pos"], asm["record"], asm["names"])
        eng.build_graph()
        got = eng.synteny_blocks(1, 0, max_gap=case["max_gap"], min_anchors=case["min_anchors"], query_length=case["lengths"][1],
                                 subject_length=case["lengths"][0])
        assert (got["n_anchors_total"], got["n_links"]) == (case["n_anchors_total"], case["n_links"])
        for name in R.FIELDS:
            assert np.array_equal(got[name].astype(np.int64), case["expect"][name]), name
        res = eng.synteny_assess()
    want = A.assess(as_tuples(got), case["k"], case["lengths"][1].tolist(), case["lengths"][0].tolist())
    assert (want["n_chains"], want["covered_subject"], want["chained_subject"]) == (case["n_chains"], case["covered_subject"], case["chained_subject"])
    for key in SCALARS:
        assert res[key] == want[key], (key, res[key], want[key])
    for name in A.CHAIN_FIELDS:
        assert np.array_equal(res["chains"][name].astype(np.int64), np.array(want["chains"][name], dtype=np.int64)), "chain " + name
    for name in A.BP_FIELDS:
        assert np.array_equal(res["bps"][name].astype(np.int64), np.array(want["bps"][name], dtype=np.int64)), "breakpoint " + name
    print(f"cover of {case['n_chains']} chains: {time.time() - t0:.1f} s")


def test_piece_tables():
    "1000 pieces in one record, a piece per record, GAP pieces only"
    case = AC.row_case(600, "mixed", seed=5)
    lengths = case["lengths"][1]
    with load(case) as eng:
        # (record 0 holds blocks 0 .. 199, each inside [300 b, 300 b + 132): five cuts in every space between two of them, four in the tail)
        at = [0] + sorted({300 * b + d for b in range(199) for d in (140, 150, 160, 170, 180)} | {lengths[0] - d for d in (1, 2, 3, 4)}) + [lengths[0]]
        many = [(0, lo, hi, A_FWD) for lo, hi in zip(at, at[1:])]
        assert len(many) == 1000
        _, want = check(eng, case, pieces=many, first=[0, 1000])
        assert want["n_chains"] > 1 and sum(want["breakpoints"][(kind, 1)] for kind in range(3)) > 0
        check(eng, case, pieces=many, first=[0, 1000], assess=dict(join_indel=1))
        _, want = check(eng, case, pieces=[(r, 0, ln, r % 2) for r, ln in enumerate(lengths)], first=list(range(len(lengths) + 1)))
        assert sum(want["breakpoints"][(kind, 1)] for kind in range(3)) == 0
        blocks, want = check(eng, case, pieces=[(0, 0, 10, A_GAP), (0, 0, 500, A_GAP), (0, 0, 7, A_GAP)], first=[0, 2, 3])
        assert blocks["n_blocks"] == want["n_chains"] == 0 and want["query_bases"] == 517 and want["ng"]["l50"] == 0


def test_parameters_at_zero_and_a_raised_filter():
    case = AC.row_case(900, "mixed", seed=9)
    with load(case) as eng:
        n_chains = [check(eng, case, assess=params)[1]["n_chains"] for params in (dict(), dict(merge_gap=0), dict(max_indel=0), dict(join_indel=0),
                                                                                   dict(merge_gap=0, max_indel=0, join_indel=0))]
        assert n_chains[2] < n_chains[0] and n_chains[4] <= n_chains[2]
        blocks, _ = check(eng, case, min_anchors=3)
        assert 0 < blocks["n_blocks"] < 900


def test_three_assemblies():
    "the third assembly holds every minimizer in the query's own order: against it every query record is one chain"
    case = cases.from_anchors(_anchors_of(AC.row_case(700, "mixed", seed=4)), extra_asm=True, max_gap=100)
    case["assess"] = {}
    with load(case) as eng:
        _, a = check(eng, case, q=1, s=0)
        _, b = check(eng, case, q=1, s=2, max_gap=0)
        _, c = check(eng, case, q=0, s=1)
    assert a["n_chains"] > 1 and b["n_breakpoints"] == 0 and c["n_chains"] > 1


def _anchors_of(case):
    "the anchors (qrec, qpos, srec, spos) of a two-assembly case, from its assemblies"
    where = {}
    for r, (_rid, mxs) in enumerate(case["asms"][0]):
        for hsh, pos in mxs:
            where[hsh] = (r, pos)
    return [(r, pos) + where[hsh] for r, (_rid, mxs) in enumerate(case["asms"][1]) for hsh, pos in mxs]


def test_refusals_leave_the_handle_usable(tmp_path):
    from ntjoin_amd import capi
    from ntjoin_amd.engine import MxEngine, MxError
    case, _ = ANCHOR["union"]
    with MxEngine(k=32, w=10) as eng:   # no blocks call before
        with pytest.raises(MxError) as err:
            eng.synteny_assess()
        assert err.value.code == capi.MXG_EINVAL and "mxg_synteny_blocks" in str(err.value)
    with load(case) as eng:
        with pytest.raises(MxError) as err:
            eng.synteny_assess()
        assert err.value.code == capi.MXG_EINVAL
        with pytest.raises(MxError):   # a failed blocks call leaves no blocks
            eng.synteny_blocks(1, 0, min_anchors=1, query_length=case["lengths"][1], subject_length=case["lengths"][0])
        with pytest.raises(MxError) as err:
            eng.synteny_assess()
        assert err.value.code == capi.MXG_EINVAL
        device(eng, case)
        p, v = capi.AssessParams(C.sizeof(capi.AssessParams), 100000, 1000, 100000), capi.AssessView()
        lib, h = eng._lib, eng._h
        assert lib.mxg_synteny_assess(h, None, C.byref(v)) == capi.MXG_EINVAL and b"null" in lib.mxg_last_error(h)
        assert lib.mxg_synteny_assess(h, C.byref(p), None) == capi.MXG_EINVAL
        assert lib.mxg_synteny_assess(None, C.byref(p), C.byref(v)) == capi.MXG_EINVAL
        p.struct_size = 12
        assert lib.mxg_synteny_assess(h, C.byref(p), C.byref(v)) == capi.MXG_EINVAL and b"struct_size" in lib.mxg_last_error(h)
        _, want = check(eng, case)
        assert want["covered_subject"] == 568
        g = eng.get_graph()
        assert g["vertex_pos"].shape[0] == 2 and eng.sketch_size(0) == g["vertex_pos"].shape[1]   # graph and sketches as they were


def test_paf_is_the_same_after_an_assess_call(tmp_path):
    case = AC.row_case(1500, "mixed", seed=2)
    with load(case) as eng:
        device(eng, case)
        eng.write_synteny_paf(tmp_path / "before.paf")
        eng.synteny_assess()
        eng.synteny_assess(merge_gap=0)
        eng.write_synteny_paf(tmp_path / "after.paf")
    assert (tmp_path / "before.paf").read_bytes() == (tmp_path / "after.paf").read_bytes() and (tmp_path / "before.paf").stat().st_size > 50000
