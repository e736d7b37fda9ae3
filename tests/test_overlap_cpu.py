"""Overlap stage, CPU side: the restatement of the reference's contract (tests/_overlap_restatement.py) is
held to every golden under tests/golden/overlap (the reference's own output, tests/golden/make_golden_overlap.py), the three
path strings the reference's tests pin come out of the recorded adjustments, and the C symbol is declared and bound."""
import glob
import os
import re

import pytest

from tests import _oracle, _overlap_cases as cases, _overlap_restatement as rs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
CASES = sorted(glob.glob(os.path.join(GOLDEN, "overlap", "*.json")))


def load_case(path):
    doc, fasta = cases.load_case(path)
    seqs = dict(_oracle.read_fasta(fasta))
    paths = [[(nd[0], nd[1], nd[2], nd[3], nd[8]) for nd in path] for path in doc["paths"]]
    return doc, seqs, paths


def oracle_sketch():
    orc = _oracle.load()
    return lambda text, k, w: [(h, p) for h, p, _f, _m in orc.sketch(text, k, w)]


def test_cases_present():
    names = {os.path.basename(c) for c in CASES}
    assert {"f-f.overlapping.json", "f-r.overlapping.json", "r-r.overlapping.json", "synth_k15_w10.json"} <= names


@pytest.mark.parametrize("case", CASES, ids=[os.path.basename(c)[:-5] for c in CASES])
def test_restatement_equals_golden(case):
    doc, seqs, paths = load_case(case)
    sa, ea, cf, _ = rs.cuts(paths, seqs, doc["meta"]["k"], doc["meta"]["w"], oracle_sketch())
    assert sa == doc["start_adjust"]
    assert ea == doc["end_adjust"]
    assert cf == doc["cut_found"]


@pytest.mark.parametrize("name,want", [("f-f.overlapping", "1+:0-2033 20N 2+:34-2331"), ("f-r.overlapping", "1+:0-2033 20N 2-:0-2297"),
                                       ("r-r.overlapping", "1-:66-2099 20N 2-:0-2297")])
def test_reference_path_strings(name, want):
    "what the reference's tests assert of its .path file (tests/ntjoin_test.py:199-221), from the recorded adjustments"
    doc, _, _ = load_case(os.path.join(GOLDEN, "overlap", name + ".json"))
    assert len(doc["paths"]) == 1
    assert rs.path_string(doc["paths"][0], doc["start_adjust"][0], doc["end_adjust"][0]) == want == doc["meta"]["reference_path"]


def test_synthetic_set_covers_the_contract():
    "the shares the generator asserts, re-asserted on the committed file"
    doc, seqs, paths = load_case(os.path.join(GOLDEN, "overlap", "synth_k15_w10.json"))
    _, _, cf, kinds = rs.cuts(paths, seqs, 15, 10, oracle_sketch())
    n = {"run": 0, "single": 0, "none": 0}
    junctions = overlapping = cut = even = 0
    pairs = set()
    for path, kd, found in zip(paths, kinds, doc["cut_found"]):
        assert 2 <= len(path) <= 20
        for i in range(len(path) - 1):
            junctions += 1
            pairs.add(path[i][1] + path[i + 1][1])
            if path[i][4] < 0:
                overlapping += 1
                kind, length, differs = kd[i]
                n[kind] += 1
                cut += found[i]
                even += kind == "run" and length % 2 == 0 and differs
    assert junctions >= 200 and pairs == {"++", "+-", "-+", "--"}
    assert 2 * cut >= overlapping
    assert min(n.values()) >= 10 and even >= 10
    assert any(len(p) == 20 for p in paths) and any(len(p) == 2 for p in paths)
    lens_gaps = [(nd[3] - nd[2], nd[4]) for p in paths for nd in p]
    assert any(-g > ln for ln, g in lens_gaps) and any(g == -1 for _, g in lens_gaps) and any(g < -2500 for _, g in lens_gaps)
    assert any("N" in seqs[nd[0]] for p in paths for nd in p)
    assert sum(os.path.getsize(c) for c in CASES) < 64 * 1024


def test_string_order_is_not_numeric_order():
    "(of the restatement alone; the kernel's string order is held by the goldens' even runs, tests/test_gpu_overlap.py)"
    src = [(9, 100), (10, 110)]
    tgt = [(9, 5), (10, 15)]
    # the walk starts at "10" (< "9" as strings): mid = walk[1] = 9
    assert rs.junction_cut(src, tgt, 120, -30)[:2] == (100, 5)


def test_symbol_declared_and_bound():
    from ntjoin_amd import capi
    with open(os.path.join(REPO, "include", "ntjoin_mx.h"), encoding="utf-8") as fh:
        header = fh.read()
    assert "mxg_overlap_cuts" in capi.SYMBOLS and re.search(r"\bint mxg_overlap_cuts\(", header)
    assert int(re.search(r"#define MXG_ABI_VERSION (\d+)", header).group(1)) == capi.ABI_VERSION
    assert hasattr(capi.load(), "mxg_overlap_cuts")
