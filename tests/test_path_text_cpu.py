"""CPU tests of the .path / AGP text (row f8) and of the scaffolder's command line: the restatement (tests/_path_text_restatement.py)
against the goldens and the AGP lines the reference's own tests pin, its two formulations against each other on seeded random
cases, and what `python -m ntjoin_amd.assemble` and `ntJoin-mx scaffold` decide before any engine exists."""
import glob
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from ntjoin_amd import assemble, capi, run
from tests import _oracle, _path_text_restatement as pt, _scaffold_cases as cases, _scaffold_pin as pin, _scaffold_restatement as rs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(glob.glob(os.path.join(cases.GOLDEN, "scaffolds", "*.json")))
IDS = [os.path.basename(c)[:-5] for c in CASES]

# the AGP lines pinned in tests/test_gpu_scaffolds.py (the lines the reference's own AGP tests expect)
PINNED_AGP = {
    "f-f.termN.unassigned": ["ntJoin0\t1\t1981\t1\tW\t1_f\t5\t1985\t+", "ntJoin0\t1982\t2001\t2\tN\t20\tscaffold\tyes\talign_genus",
                             "ntJoin0\t2002\t4330\t3\tW\t2_f\t1\t2329\t+", "unassigned:0-14\t1\t8\t1\tW\tunassigned\t3\t10\t+"],
    "f-r.overlapping": ["ntJoin0\t1\t2033\t1\tW\t1\t1\t2033\t+", "ntJoin0\t2034\t2053\t2\tN\t20\tscaffold\tyes\talign_genus",
                        "ntJoin0\t2054\t4350\t3\tW\t2\t1\t2297\t-"],
}


def golden_inputs(case):
    "-> (paths, leads, tails, unassigned intervals with their strips, first line) of a golden, the strips from the scaffold restatement"
    doc, fasta = cases.load_golden(case)
    records = _oracle.read_fasta(fasta)
    seqs = dict(records)
    paths = cases.golden_nodes(doc)
    _text, leads, tails = rs.scaffolds(paths, seqs, doc["meta"]["overlap_gap"] if doc["meta"]["overlap"] else None)
    bed, _fa, _n = rs.unassigned(records, paths)
    unassigned = []
    for line in bed.splitlines():
        rid, lo, hi = line.split("\t")
        text = seqs[rid][int(lo):int(hi)]
        lead = len(text) - len(text.lstrip("Nn"))
        unassigned.append((rid, int(lo), int(hi), lead, 0 if lead == len(text) else len(text) - len(text.rstrip("Nn"))))
    return doc, paths, leads, tails, unassigned, doc["meta"]["fasta"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_gives_the_goldens_path_text(case):
    doc, paths, leads, tails, unassigned, first_line = golden_inputs(case)
    text, agp = pt.by_regex(paths, leads, tails, first_line, unassigned)
    assert text == doc["path"]
    assert (text, agp) == pt.direct(paths, leads, tails, first_line, unassigned)
    name = os.path.basename(case)[:-5]
    if name in PINNED_AGP:
        assert agp.splitlines() == PINNED_AGP[name]


def test_both_pinned_agp_cases_are_among_the_goldens():
    assert set(PINNED_AGP) <= set(IDS)


TRICKY_IDS = ["c", "ab", "x+:12-34", "+:12-34", "a-", "-", "a:b", ":", "12", "7-9", "r+:1-2+:3-4", "id-:5-6x", "N", "20N", "9N+", "a.b|c_d",
              "x" * 300]


def random_case(seed):
    """paths, leads, tails: coordinates and gaps at the digit borders, all four combinations of cuts, strips on end nodes long enough
    to keep text behind them (the cuts stay 20 bases clear of either end there), so that no interval comes out empty or inverted"""
    rng = random.Random(seed)
    paths, leads, tails = [], [], []
    for _ in range(rng.randint(1, 12)):
        path = []
        for _i in range(rng.choice([2, 2, 3, 5, 9])):
            start = rng.choice([0, 0, 1, 9, 10, 99, 100, 12345, 999999999, 4294967000])
            length = rng.choice([1, 2, 9, 10, 95, 1000, 4000000000]) if start < 1000 else rng.randint(1, 290)
            room = 20 if length >= 100 else 0
            kind = rng.randrange(4)
            ea = rng.randint(1 + room, length - room) if kind & 2 else 0
            sa = rng.randint(0, (ea if ea else length - room) - 1) if kind & 1 else 0
            path.append((rng.choice(TRICKY_IDS), rng.choice("+-"), start, start + length, rng.choice([0, 0, 1, 9, 10, 20, 99, 100, 4294967295]), sa, ea))
        paths.append(path)
        leads.append(rng.choice([0, 0, 1, 7]) if path[0][3] - path[0][2] >= 100 else 0)
        tails.append(rng.choice([0, 0, 2, 11]) if path[-1][3] - path[-1][2] >= 100 else 0)
    return paths, leads, tails


def test_fields_formatted_directly_equal_the_regex_round_trip():
    """300 seeded cases with ids that contain `+:12-34`, '-', ':' and digits: the greedy (\\S+) of the reference's expression always
    recovers the true trailing fields, so the device formats the AGP from the node's fields and skips the round trip"""
    seen_ids, seen_cuts = set(), set()
    for seed in range(300):
        paths, leads, tails = random_case(seed)
        unassigned = [("u+:1-2", 0, 14, 2, 4), ("allN", 3, 9, 6, 0), ("k", 5, 4000000000, 0, 1)] if seed % 2 else None
        assert pt.by_regex(paths, leads, tails, "t.fa", unassigned) == pt.direct(paths, leads, tails, "t.fa", unassigned), seed
        seen_ids |= {nd[0] for path in paths for nd in path}
        seen_cuts |= {(nd[1], nd[5] > 0, nd[6] > 0) for path in paths for nd in path}
    assert seen_ids == set(TRICKY_IDS) and len(seen_cuts) == 8


def test_a_sum_beyond_32_bits_and_a_gap_of_zero():
    "three nodes of 4 * 10^9 bases each print 12 000 000 000; a gap of 0 in the middle keeps its line, ending at at - 1"
    big = 4000000000
    paths = [[("a", "+", 0, big, 0, 0, 0), ("b", "-", 5, big + 5, 7, 0, 0), ("c", "+", 0, big, 0, 0, 0)]]
    text, agp = pt.direct(paths, [0], [0], "t.fa")
    assert (text, agp) == pt.by_regex(paths, [0], [0], "t.fa")
    lines = agp.splitlines()
    assert lines[1] == f"ntJoin0\t{big + 1}\t{big}\t2\tN\t0\tscaffold\tyes\talign_genus"
    assert lines[-1] == f"ntJoin0\t{2 * big + 8}\t12000000007\t5\tW\tc\t1\t{big}\t+"
    assert text == f"t.fa\nntJoin0\ta+:0-{big} 0N b-:5-{big + 5} 7N c+:0-{big}\n"


# ---- the command line, before any engine exists ---------------------------------------------------------------------------

def test_assemble_takes_run_s_parser_and_the_capi_names_the_call():
    assert assemble.parse_arguments is run.parse_arguments and assemble.set_weights is run.set_weights
    assert "mxg_write_paths" in capi.SYMBOLS and capi.PATHS_AGP_UNASSIGNED == 1
    with open(os.path.join(REPO, "include", "ntjoin_mx.h"), encoding="utf-8") as fh:
        header = fh.read()
    assert re.search(r"\bint mxg_write_paths\(", header) and "#define MXG_PATHS_AGP_UNASSIGNED 0x1u" in header
    for cite in ("bin/ntjoin_assemble.py:605-610", ":346-376", ":379-404", "bin/path_node.py:41-61"):
        assert cite in header


def test_names_are_derived_from_the_sketches_names(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    args = run.parse_arguments(["-s", "dir/t.fa.k32.w500.tsv", "-r", "2 3", "-k", "32", "a.fa.k32.w500.tsv", "b.k9.fa.k32.w500.tsv"])
    fasta, w = assemble.derive_names(args)
    assert w == 500
    assert fasta == {"dir/t.fa.k32.w500.tsv": "dir/t.fa", "a.fa.k32.w500.tsv": "a.fa", "b.k9.fa.k32.w500.tsv": "b.k9.fa"}
    os.mkdir("dir")
    for name in ("dir/t.fa", "a.fa", "b.k9.fa", "b.k9.fa.k32.w500.tsv"):
        with open(name, "w", encoding="ascii") as fh:
            fh.write(">x\nACGT\n")
    # the target is always sketched; a reference only when its TSV does not exist
    assert assemble.sources(args, fasta) == {"dir/t.fa.k32.w500.tsv": "dir/t.fa", "a.fa.k32.w500.tsv": "a.fa"}


@pytest.mark.parametrize("argv,message", [
    (["-s", "t.fa.tsv", "-r", "2", "-k", "32", "a.fa.k32.w500.tsv"], "is not named <fasta>.k<k>.w<w>.tsv"),
    (["-s", "t.fa.k32.w500.tsv", "-r", "2", "-k", "24", "a.fa.k24.w500.tsv"], "names k=32 but -k is 24"),
    (["-s", "t.fa.k32.w500.tsv", "-r", "2", "-k", "32", "a.fa.k32.w1000.tsv"], "different window sizes"),
    (["-s", "t.fa.k32.w500.tsv", "-r", "2", "-k", "32", "missing.fa.k32.w500.tsv"], "neither the sketch 'missing.fa.k32.w500.tsv' nor the FASTA"),
], ids=["name", "k", "w", "no-source"])
def test_bad_command_lines_end_with_error_and_status_1(argv, message, tmp_path):
    "in a child process: one line on stdout that starts with ERROR:, status 1, and no library loaded on the way (there is no GPU here)"
    with open(tmp_path / "t.fa", "w", encoding="ascii") as fh:
        fh.write(">x\nACGT\n")
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""), MXG_LIB_DIR=str(tmp_path / "no_such_build"))
    res = subprocess.run([sys.executable, "-m", "ntjoin_amd.assemble"] + argv, cwd=tmp_path, env=env, capture_output=True, text=True, check=False)
    assert res.returncode == 1, res.stderr
    lines = res.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith("ERROR: ") and message in lines[0]
    assert sorted(os.listdir(tmp_path)) == ["t.fa"]


def make_n(*words):
    res = subprocess.run(["make", "-n", "-f", os.path.join(REPO, "ntJoin-mx")] + list(words), capture_output=True, text=True, check=False)
    assert res.returncode == 0, res.stderr
    return " ".join(res.stdout.replace("\\\n", " ").split())


def test_make_scaffold_forwards_every_variable_and_concatenates():
    out = make_n("scaffold", "target=t.fa", "references=a.fa b.fa", "reference_weights=2 3", "target_weight=4", "k=24", "w=250", "n=2", "prefix=pre",
                 "g=7", "G=900", "m=80", "mkt=True", "agp=True", "no_cut=True", "overlap_k=11", "overlap_w=12", "overlap_g=13", "assemble_t=3", "t=6")
    assert "python3 -m ntjoin_amd.assemble -p pre -n 2 -s t.fa.k24.w250.tsv -l 4 -r \"2 3\" -k 24 -g 7 -G 900 -m 80 -t 3 --mkt --no_cut --agp " \
           "--overlap --overlap_gap 13 --btllib_t 6 --overlap_k 11 --overlap_w 12 a.fa.k24.w250.tsv b.fa.k24.w250.tsv" in out
    assert out.endswith("cat t.fa.k24.w250.n2.assigned.scaffolds.fa t.fa.k24.w250.n2.unassigned.scaffolds.fa > t.fa.k24.w250.n2.all.scaffolds.fa")
    assert f"PYTHONPATH={REPO}:" in out


def test_make_scaffold_has_the_reference_s_defaults_and_needs_no_checkout():
    out = make_n("scaffold", "target=t.fa", "references=a.fa", "reference_weights=2")
    assert "-p out.k32.w1000.n1 -n 1 -s t.fa.k32.w1000.tsv -l 1 -r \"2\" -k 32 -g 20 -G 0 -m 90 -t 1 --overlap --overlap_gap 20 --btllib_t 4 " \
           "--overlap_k 15 --overlap_w 10 a.fa.k32.w1000.tsv" in out
    off = make_n("scaffold", "target=t.fa", "references=a.fa", "reference_weights=2", "overlap=False", "g=33")
    assert "--overlap" not in off and "--agp" not in off and "--mkt" not in off and "--no_cut" not in off and "-g 33" in off
    on = make_n("scaffold", "target=t.fa", "references=a.fa", "reference_weights=2", "g=33")
    assert "--overlap_gap 33" in on  # overlap_g follows g, as in the reference
    assert "scaffold" in make_n("help")


# ---- the families of tests/golden/scaffolds/families: the reference's own .path, write_agp and write_agp_unassigned -----------------

PIN_CASES = pin.all_cases()
PIN_IDS = [f"{family}-{name}" for family, name in PIN_CASES]


@pytest.mark.parametrize("family,name", PIN_CASES, ids=PIN_IDS)
def test_both_formulations_give_the_reference_s_path_and_agp(family, name):
    """by_regex: every pinned path, the inverted intervals and their negative lengths included, and the unassigned lines; direct: the
    same text over the paths it does not refuse, and a refusal that names the path and node for each of the others"""
    entry = pin.load_family(family)[name]
    case, paths = entry["case"], entry["paths"]
    _text, leads, tails = rs.scaffolds(paths, dict(case["records"]), case["overlap_gap"])
    unassigned = pin.unassigned_intervals(case, paths)
    assert pt.by_regex(paths, leads, tails, pin.TARGET[:4], unassigned) == (entry["path"], entry["agp"] + entry["agp_unassigned"])
    refused = pin.refused_nodes(entry)
    keep = [q for q in range(len(paths)) if q not in refused]
    want = pin.renumbered(entry, keep)
    assert pt.direct([paths[q] for q in keep], [leads[q] for q in keep], [tails[q] for q in keep], pin.TARGET[:4]) == want
    if not refused:
        assert pt.direct(paths, leads, tails, pin.TARGET[:4], unassigned) == (entry["path"], entry["agp"] + entry["agp_unassigned"])
    for q, i in refused.items():
        with pytest.raises(pt.Refused, match=f"path 0 node {i}: the adjusted interval is empty or inverted"):
            pt.direct([paths[q]], [leads[q]], [tails[q]], pin.TARGET[:4])
        assert any(int(line.split("\t")[2]) < int(line.split("\t")[1]) for line in entry["agp_lines"][q])  # the reference prints them


def test_the_reference_s_round_trip_keeps_every_id_of_agp_names():
    "finding of the agp_names family: write_agp's two expressions recover all six ids, '+:1-' and '-:7-9' inside them included"
    for entry in pin.load_family("agp_names").values():
        for path, lines in zip(entry["paths"], entry["agp_lines"]):
            assert [line.split("\t")[5] for line in lines[::2]] == [nd[0] for nd in path]
            assert [line.split("\t")[8] for line in lines[::2]] == [nd[1] for nd in path]


@pytest.mark.parametrize("family,name", PIN_CASES, ids=PIN_IDS)
def test_the_host_loop_gives_the_reference_s_path_and_agp(family, name, tmp_path):
    "Ntjoin._write_path_host, the route print_scaffolds takes when the writer refuses a path: every pinned path, inverted intervals included"
    from ntjoin_amd.ntjoin import Ntjoin
    entry = pin.load_family(family)[name]
    case, paths = entry["case"], entry["paths"]
    _text, leads, tails = rs.scaffolds(paths, dict(case["records"]), case["overlap_gap"])
    unassigned = pin.unassigned_intervals(case, paths)

    class Strips:
        "the one call the host loop makes on the engine"
        @staticmethod
        def scaffold_strips():
            return np.array([u[3] for u in unassigned], dtype=np.uint32), np.array([u[4] for u in unassigned], dtype=np.uint32)

    nj = Ntjoin.__new__(Ntjoin)
    nj._engine = Strips()
    files = {kind: str(tmp_path / ("out." + kind)) for kind in ("path", "agp", "bed")}
    with open(files["bed"], "w", encoding="ascii") as fh:
        fh.write(rs.unassigned(case["records"], paths)[0])
    nj._write_path_host(files, pin.TARGET[:4], [(pin.rows9(path), [(nd[5], nd[6]) for nd in path]) for path in paths], leads, tails)
    with open(files["path"], encoding="ascii") as fh:
        assert fh.read() == entry["path"]
    with open(files["agp"], encoding="ascii") as fh:
        assert fh.read() == entry["agp"] + entry["agp_unassigned"]
