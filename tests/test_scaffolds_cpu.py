"""Scaffold stage, CPU side: the restatement of the contract (tests/_scaffold_restatement.py) is held to every
golden under tests/golden/scaffolds (the reference's own print_scaffolds output, tests/golden/make_golden_scaffolds.py) and to the
four result files the reference's tests hold for the f-f run, and to the reference's answers on the generated families
(tests/golden/scaffolds/families, tests/golden/make_golden_scaffold_fuzz.py), whose conditions are recomputed here; the fuzz cases of the GPU test cover what they must and leave out no
more than their cap; the symbol is in the header and in the built library; a TSV-loaded target is refused by name."""
import argparse
import glob
import os
import re

import pytest

from ntjoin_amd import capi
from tests import _scaffold_cases as cases, _scaffold_pin as pin, _scaffold_restatement as rs
from tests import _oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(glob.glob(os.path.join(cases.GOLDEN, "scaffolds", "*.json")))
IDS = [os.path.basename(c)[:-5] for c in CASES]
EXPECTED = os.path.join(cases.GOLDEN, "scaffolds", "expected_f-f")


def test_the_goldens_are_the_issue_s_cases():
    assert set(IDS) == {"f-f", "f-f.termN", "f-f.termN.unassigned", "f-f.overlapping", "f-r.overlapping", "r-r.overlapping"}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_equals_golden(case):
    doc, fasta = cases.load_golden(case)
    records = _oracle.read_fasta(fasta)
    paths = cases.golden_nodes(doc)
    gap = doc["meta"]["overlap_gap"] if doc["meta"]["overlap"] else None
    text, leads, tails = rs.scaffolds(paths, dict(records), gap)
    assert text == doc["assigned"]
    assert rs.path_text(doc["meta"]["fasta"], paths, leads, tails) == doc["path"]
    if "termN" in case:
        assert leads == [4] and tails == [0]
    if doc["meta"]["overlap"]:
        assert any(sa or ea for path in paths for *_, sa, ea in path)


def test_restatement_equals_the_reference_s_expected_outputs():
    doc, fasta = cases.load_golden(os.path.join(cases.GOLDEN, "scaffolds", "f-f.json"))
    records = _oracle.read_fasta(fasta)
    paths = cases.golden_nodes(doc)
    text, leads, tails = rs.scaffolds(paths, dict(records), None)
    bed, un_fa, n = rs.unassigned(records, paths)
    want = {}
    for f in os.listdir(EXPECTED):
        with open(os.path.join(EXPECTED, f), encoding="ascii") as fh:
            want[f] = fh.read()
    assert text == want["scaf.f-f.fa.k32.w1000.n1.assigned.scaffolds.fa"]
    assert un_fa == want["scaf.f-f.fa.k32.w1000.n1.unassigned.scaffolds.fa"] and n == 0
    assert bed == want["f-f_test.scaf.f-f.fa.k32.w1000.tsv.unassigned.bed"]
    assert rs.path_text("scaf.f-f.fa", paths, leads, tails) == want["f-f_test.path"]


def test_unassigned_of_the_termn_fixture():
    "the record no path takes: bedtools' interval keeps its coordinates, its text loses the Ns (the reference's AGP test: unassigned:0-14, bases 3-10)"
    doc, fasta = cases.load_golden(os.path.join(cases.GOLDEN, "scaffolds", "f-f.termN.unassigned.json"))
    records = _oracle.read_fasta(fasta)
    bed, un_fa, n = rs.unassigned(records, cases.golden_nodes(doc))
    assert "unassigned\t0\t14\n" in bed and n >= 1
    m = re.search(r">unassigned:0-14\n(\S+)\n", un_fa)
    assert m and len(m.group(1)) == 8


def test_restatement_refuses_what_the_library_refuses():
    seqs = {"a": "NNACGTNN", "b": "ACGTACGT", "n": "NNNN"}
    ok = [("a", "+", 0, 8, 3, 0, 0), ("b", "-", 0, 8, 0, 0, 0)]
    text, leads, tails = rs.scaffolds([ok], seqs)
    assert text == ">ntJoin0\nACGTNNNNNACGTACGT\n" and leads == [2] and tails == [0]
    for bad in ([ok[0]], [("n", "+", 0, 4, 0, 0, 0), ok[1]], [ok[0], ("n", "-", 1, 3, 0, 0, 0)], [("a", "+", 3, 3, 0, 0, 0), ok[1]],
                [("a", "+", 0, 9, 0, 0, 0), ok[1]]):
        with pytest.raises(rs.Refused):
            rs.scaffolds([bad], seqs)
    with pytest.raises(rs.Refused):
        rs.scaffolds([[("a", "+", 0, 8, 0, 0, 9), ok[1]]], seqs, 20)
    with pytest.raises(rs.Refused):
        rs.scaffolds([[("a", "+", 0, 8, 0, 5, 5), ok[1]]], seqs, 20)
    # the reverse complement's table: IUPAC codes and U, both cases, anything else unchanged
    assert rs.oriented("ACGTUNMRWSYKVHDBacgtunmrwsykvhdb*x", "-", 0, 34) == "x*vhdbmrswyknaacgtVHDBMRSWYKNAACGT"


def test_fuzz_cases_cover_the_contract_and_stay_under_their_cap():
    feats, generated, left_out = set(), 0, 0
    for seed in cases.FUZZ_SEEDS:
        case = cases.fuzz_case(seed)
        feats |= case["features"]
        generated += case["generated"]
        left_out += case["left_out"]
        assert case["paths"], seed
    assert not (cases.REQUIRED_FEATURES - feats), sorted(cases.REQUIRED_FEATURES - feats)
    assert left_out <= cases.MAX_LEFT_OUT * generated, (left_out, generated)


def test_symbol_in_header_and_library():
    with open(os.path.join(REPO, "include", "ntjoin_mx.h"), encoding="utf-8") as fh:
        header = fh.read()
    assert "mxg_write_scaffolds" in capi.SYMBOLS and re.search(r"\bint mxg_write_scaffolds\(", header)
    assert "bin/ntjoin_assemble.py:580-613" in header and "typedef struct mxg_scaffold_node" in header
    assert hasattr(capi.load(), "mxg_write_scaffolds")
    from ntjoin_amd.engine import MxEngine
    assert MxEngine.SCAFFOLD_NODE.itemsize == 28


def test_print_scaffolds_refuses_a_tsv_target_before_anything_runs():
    "(no handle is needed to say so: the check reads what the Ntjoin was given)"
    from ntjoin_amd.ntjoin import Ntjoin
    nj = object.__new__(Ntjoin)
    nj._engine, nj._order, nj._fasta = None, ["t.fa.k32.w100.tsv"], {}
    nj.args = argparse.Namespace(p="out")
    with pytest.raises(ValueError, match="TSV.*FASTA"):
        nj.print_scaffolds([])


# ---- the families of tests/golden/scaffolds/families: generated inputs, the reference's own print_scaffolds ------------------------

PIN_CASES = pin.all_cases()
PIN_IDS = [f"{family}-{name}" for family, name in PIN_CASES]


@pytest.mark.parametrize("family,name", PIN_CASES, ids=PIN_IDS)
def test_restatement_equals_the_reference_on_the_families(family, name):
    "every pinned path: the scaffold's name, length and digest, the .path line, and the strips the reference's coordinates show"
    entry = pin.load_family(family)[name]
    case = entry["case"]
    text, leads, tails = rs.scaffolds(entry["paths"], dict(case["records"]), case["overlap_gap"])
    assert pin.scaffold_digests(text) == entry["scaffolds"]
    assert rs.path_text(pin.TARGET[:4], entry["paths"], leads, tails) == entry["path"]
    assert list(zip(leads, tails)) == [pin.reference_strips(path, line) for path, line in zip(entry["paths"], entry["path_lines"])]


@pytest.mark.parametrize("family", pin.FAMILIES)
def test_the_families_hold_what_their_readme_promises(family):
    "the conditions of tests/golden/scaffolds/families/README.md, recomputed from the committed files; no file beyond the size limit"
    found = pin.check_conditions(family, pin.load_family(family))
    assert found["pinned"] + found["raised"] == found["generated"]
    for f in os.listdir(pin.FAMILY_DIR):
        assert os.path.getsize(os.path.join(pin.FAMILY_DIR, f)) <= 720_100, f


def test_the_family_fuzz_is_the_gpu_fuzz_with_the_fold_off():
    for seed in (1, 2, 47):
        ours, theirs = pin.fuzz_case(seed), cases.fuzz_case(seed)
        assert all(ours[key] == theirs[key] for key in ours)
    assert [args["seed"] for _n, _g, args in pin.family_specs()["fuzz"]] == cases.FUZZ_SEEDS
