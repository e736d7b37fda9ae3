#!/usr/bin/env python3
"""Goldens of the scaffold stage (tests/golden/scaffolds/*.json).  BUILD CONTAINER ONLY, like make_golden.py and
make_golden_overlap.py: it reads the reference tree, and it only imports it.

The reference's OWN print_scaffolds (bin/ntjoin_assemble.py:530-626) runs with print_unassigned stubbed (that one needs pybedtools
and the bedtools binary) on PathNodes made from what its own format_path returned (recorded under tests/golden/cases and
tests/golden/overlap).  With the overlap stage on it computes the cuts itself (adjust_for_trimming over the btllib and igraph
stand-ins of make_golden_overlap.py); they are checked against the recorded cuts of tests/golden/overlap.  Recorded per case: the
nodes, the adjustments, the assigned FASTA and the .path text.

Cases: the f-f fixture at n = 1 with the overlap stage off; the two termN fixtures likewise (the strip of terminal Ns); the three
*.overlapping.fa fixtures with the overlap stage on and overlap_gap = 20.

The unassigned side is pinned by results the reference's tests hold: the f-f run's assigned and unassigned FASTA, .path and
.unassigned.bed are copied as data files from its tests/expected_outputs/ into tests/golden/scaffolds/expected_f-f/."""
import collections
import contextlib
import io
import json
import os
import shutil
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_overlap as mgo  # noqa: E402
from tests import _oracle  # noqa: E402

OUT = os.path.join(HERE, "scaffolds")
FASTA = os.path.join(HERE, "fasta")
EXPECTED = ["scaf.f-f.fa.k32.w1000.n1.assigned.scaffolds.fa", "scaf.f-f.fa.k32.w1000.n1.unassigned.scaffolds.fa", "f-f_test.path",
            "f-f_test.scaf.f-f.fa.k32.w1000.tsv.unassigned.bed"]


def run_print_scaffolds(asm_mod, path_node, ntjoin_utils, fasta, paths9, overlap, n):
    seqs = _oracle.read_fasta(os.path.join(FASTA, fasta))
    paths = [[path_node.PathNode(*nd) for nd in path] for path in paths9]
    sc = object.__new__(asm_mod.NtjoinScaffolder)
    sc.args = types.SimpleNamespace(s=fasta + ".k32.w1000.tsv", n=n, p="out", agp=False, overlap=overlap, overlap_gap=20, overlap_k=15,
                                    overlap_w=10, btllib_t=1)
    sc.scaffolds = {rid: ntjoin_utils.Scaffold(id=rid, length=len(seq), sequence=seq) for rid, seq in seqs}
    sc.print_unassigned = lambda *a, **k: None
    cwd, tmp = os.getcwd(), tempfile.mkdtemp()
    os.chdir(tmp)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            sc.print_scaffolds(paths, {}, collections.defaultdict(set))
        with open(f"{fasta}.k32.w1000.n{n}.assigned.scaffolds.fa", encoding="ascii") as fh:
            assigned = fh.read()
        with open("out.path", encoding="ascii") as fh:
            path_text = fh.read()
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp)
    adjust = [[[nd.start_adjust, nd.end_adjust] for nd in path if nd.ori != "?"] for path in paths]
    return assigned, path_text, adjust


def main():
    if not os.path.isdir(mg.REF):
        sys.exit("make_golden_scaffolds.py needs the reference tree (build container only)")
    _oracle.build()
    orc = _oracle.load()
    mg.install_igraph_standin()
    sys.path.insert(0, os.path.join(mg.REF, "bin"))
    mgo.install_btllib_standin(orc)
    asm_mod = mg.import_scaffolder()
    import ntjoin_utils
    import path_node
    os.makedirs(OUT, exist_ok=True)

    def record(name, fasta, paths9, overlap, n, extra):
        assigned, path_text, adjust = run_print_scaffolds(asm_mod, path_node, ntjoin_utils, fasta, json.loads(json.dumps(paths9)), overlap, n)
        doc = {"meta": {"generator": "tests/golden/make_golden_scaffolds.py", "fasta": fasta, "overlap": overlap, "overlap_gap": 20, "n": n},
               "paths": paths9, "adjust": adjust, "assigned": assigned, "path": path_text}
        doc["meta"].update(extra)
        with open(os.path.join(OUT, name + ".json"), "w", encoding="ascii") as fh:
            json.dump(doc, fh, separators=(",", ":"))
            fh.write("\n")
        print(name, path_text.splitlines()[1:], len(assigned), "bytes of FASTA")
        return adjust

    for case, fasta in (("f-f_w1000", "scaf.f-f.fa"), ("f-f_termN_w1000", "scaf.f-f.termN.fa"),
                        ("f-f_termN_unassigned_w1000", "scaf.f-f.termN.unassigned.fa")):
        with open(os.path.join(HERE, "cases", case, "reference.json"), encoding="utf-8") as fh:
            paths9 = json.load(fh)["reference"]["format_by_n"]["1"]
        record(fasta.replace("scaf.", "").replace(".fa", ""), fasta, paths9, False, 1,
               {"paths_from": f"format_path as recorded in tests/golden/cases/{case} (k=32 w=1000 n=1, weights 2/1)"})
    for name in ("f-f.overlapping", "f-r.overlapping", "r-r.overlapping"):
        with open(os.path.join(HERE, "overlap", name + ".json"), encoding="ascii") as fh:
            ov = json.load(fh)
        adjust = record(name, ov["meta"]["fasta"], ov["paths"], True, 2,
                        {"paths_from": f"tests/golden/overlap/{name}.json ({ov['meta']['paths_from']})", "overlap_k": 15, "overlap_w": 10})
        want = [[list(c) for c in zip(sa, ea)] for sa, ea in zip(ov["start_adjust"], ov["end_adjust"])]
        assert adjust == want, f"{name}: print_scaffolds' own cuts differ from the recorded ones"
    exp = os.path.join(OUT, "expected_f-f")
    os.makedirs(exp, exist_ok=True)
    for f in EXPECTED:
        shutil.copyfile(os.path.join(mg.REF, "tests", "expected_outputs", f), os.path.join(exp, f))


if __name__ == "__main__":
    main()
