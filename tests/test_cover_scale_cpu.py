"""The closed form of tests/_cover_scale.py against the sequential restatements (tests/_synteny_restatement.py,
tests/_assess_restatement.py) at sizes they walk in no time: what the GPU runs with 2 524 and 263 644 chains
(tests/test_gpu_assess.py) are built from."""
import numpy as np
import pytest

from tests import _assess_cases as AC, _assess_restatement as A, _cover_scale as CS, _synteny_restatement as R

SIZES = [(0, 0), (1, 3), (7, 2), (60, 130), (401, 50)]


@pytest.mark.parametrize("m0,m1", SIZES)
def test_closed_form_is_what_the_restatements_find(m0, m1):
    case = CS.cover_scale_case(m0, m1)
    qrec, qpos, srec, spos = case["anchors"]
    want = R.synteny([spos, qpos], [srec, qrec], 1, 0, case["k"], max_gap=case["max_gap"], min_anchors=case["min_anchors"])
    assert (want["n_anchors_total"], want["n_links"]) == (case["n_anchors_total"], case["n_links"])
    assert list(zip(*[case["expect"][name].tolist() for name in R.FIELDS])) == want["blocks"]
    res = A.assess(want["blocks"], case["k"], case["lengths"][1].tolist(), case["lengths"][0].tolist())
    assert res["n_chains"] == case["n_chains"] == m0 + m1 + 2
    spans = [CS.chain_end(m) - 1000 for m in (m0, m1)]
    for at, m, span in ((0, m0, spans[0]), (m0 + 1, m1, spans[1])):   # (in the query's order the long chains stand in front of their singles)
        assert res["chains"]["n_blocks"][at] == CS.chain_blocks(m) and res["chains"]["s_end"][at] - res["chains"]["s_start"][at] == span
    assert res["covered_subject"] == case["covered_subject"] == sum(spans)
    assert res["chained_subject"] == case["chained_subject"] == sum(spans) + 82 * (m0 + m1)
    if m0 + m1:
        assert res["covered_subject"] < res["chained_subject"]
    assert res["n_breakpoints"] == max(m0 - 1, 0) + max(m1 - 1, 0) and res["breakpoints"][(A.RELOCATION, 0)] == res["n_breakpoints"]
    # the chains in the order of the assessment's sort, and the union by way of the running maximum in front of every chain
    key, word = CS.sorted_chains(m0, m1)
    c = res["chains"]
    order = sorted(range(res["n_chains"]), key=lambda i: (c["s_record"][i], c["s_start"][i]))
    assert key.tolist() == [c["s_record"][i] << 32 | c["s_start"][i] for i in order]
    assert word.tolist() == [c["s_record"][i] << 32 | c["s_end"][i] for i in order]
    assert len(set(key.tolist())) == len(key) and key[m0 + 1] == 1 << 32 | 1000   # (no two chains share a place: the order is the only one)
    before = np.concatenate([np.zeros(1, dtype=np.uint64), np.maximum.accumulate(word)[:-1]])
    assert CS.covered(key, word, before) == res["covered_subject"]


def test_it_is_cover_case_on_two_records():
    "record 0's half at m = 2900 is tests/_assess_cases.py's cover_case but for the chain's length, which here follows from m"
    mine, theirs = CS.blocks_of(2900, 0), AC.cover_case(2900)
    assert CS.chain_blocks(2900) == 59 and CS.chain_end(2900) == 12682
    specs = [(0, 200 * b, 0, 1000 + 200 * b) for b in range(59)] + [(1, 200 * j, 0, 12599 - 4 * j) for j in range(2900)]
    got = list(zip(mine["q_record"].tolist(), mine["q_start"].tolist(), mine["s_record"].tolist(), mine["s_start"].tolist()))
    assert got[:59 + 2900] == specs and theirs["n_specs"] == 2960


def test_the_input_is_a_sketch_of_each_assembly():
    case = CS.cover_scale_case(401, 50)
    for asm, lengths in zip(case["asms"], case["lengths"]):
        assert len(np.unique(asm["hash"])) == len(asm["hash"]) == case["n_anchors_total"]
        key = asm["record"].astype(np.int64) << 32 | asm["pos"].astype(np.int64)
        assert (np.diff(key) > 0).all()
        assert (asm["pos"].astype(np.int64) + case["k"] <= lengths[asm["record"]]).all() and len(lengths) == len(asm["names"])
    assert sorted(case["asms"][0]["hash"].tolist()) == sorted(case["asms"][1]["hash"].tolist())
