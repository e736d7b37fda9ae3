"""The closed form of tests/_synteny_scale.py against the sequential restatement of the contract (tests/_synteny_restatement.py), at a
size the restatement walks in no time: what the GPU run at 4.46 M anchors (tests/test_gpu_primitives.py) is compared with."""
import numpy as np
import pytest

from tests import _synteny_restatement as R, _synteny_scale as SC


@pytest.mark.parametrize("n_blocks", [1, 2, 7, 300])
def test_closed_form_is_what_the_restatement_finds(n_blocks):
    case = SC.scale_case(n_blocks)
    qrec, qpos, srec, spos = case["anchors"]
    want = R.synteny([spos, qpos], [srec, qrec], 1, 0, case["k"], max_gap=case["max_gap"], min_anchors=case["min_anchors"])
    assert (want["n_anchors_total"], want["n_links"]) == (case["n_anchors_total"], case["n_links"])
    assert list(zip(*[case["expect"][name].tolist() for name in R.FIELDS])) == want["blocks"]
    assert len(want["blocks"]) == n_blocks


def test_the_input_is_a_sketch_of_each_assembly():
    "every hash once per assembly, positions rising inside a record, records in order, every anchor inside its record's length"
    case = SC.scale_case(300)
    for asm, lengths in zip(case["asms"], case["lengths"]):
        assert len(np.unique(asm["hash"])) == len(asm["hash"]) == case["n_anchors_total"]
        key = asm["record"].astype(np.int64) << 32 | asm["pos"].astype(np.int64)
        assert (np.diff(key) > 0).all()
        assert (asm["pos"].astype(np.int64) + case["k"] <= lengths[asm["record"]]).all() and len(lengths) == len(asm["names"])
    assert sorted(case["asms"][0]["hash"].tolist()) == sorted(case["asms"][1]["hash"].tolist())
    # the blocks are dealt over all three query records and both subject records, in both directions
    e = case["expect"]
    assert set(e["q_record"].tolist()) == {0, 1, 2} and set(e["s_record"].tolist()) == {0, 1} and set(e["reverse"].tolist()) == {0, 1}
