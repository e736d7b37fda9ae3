#!/usr/bin/env python3
"""Goldens of the scaffold stage and of the .path / AGP writer on generated inputs (tests/golden/scaffolds/families/<family>.json).
BUILD CONTAINER ONLY, like its siblings: it reads the reference tree, and it only imports it.

Per case of tests/_scaffold_pin.py family_specs() (fuzz, strip_beside_cuts, agp_names) the reference's OWN print_scaffolds
(bin/ntjoin_assemble.py:530-626) runs with args.agp = True on PathNodes made from the case's nodes, their start_adjust / end_adjust
set from the case.  Stubbed: print_unassigned (pybedtools and the bedtools binary are not here); merge_relocations, as the identity
(the adjustment stage, pinned in tests/golden/adjust); and the cut step of :556-578, by an `args` whose `overlap` answers False on
its first read (:556), True on the read per path (:596) and False on the last (:624), so that the loop of :580-613 runs verbatim
over the cuts the case holds.  Every path runs alone first (one AssertionError must not hide the other paths), then the case runs
once with all paths the reference accepted, so that the recorded ntJoin<ct> numbers are its own.  The unassigned AGP lines are what
its static write_agp_unassigned writes for every line of the unassigned BED of those paths, given `<id>:<lo>-<hi>` and
seq[lo:hi] as bedtools getfasta would hand them over.

Recorded per case: meta (generator, arguments, sha256 of the input), per path "ok" or {"error": {"type", "line"}}, the .path and
.agp text verbatim, the unassigned AGP lines, and per scaffold of the assigned FASTA its name, length and the sha256 of its sequence
line.  The inputs are not written: tests/_scaffold_pin.py load_family() re-makes them.  The conditions of
tests/golden/scaffolds/families/README.md are asserted on what was recorded; a failure leaves the script with a non-zero status."""
import collections
import contextlib
import io
import json
import os
import shutil
import sys
import tempfile
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from tests import _scaffold_pin as pin  # noqa: E402
from tests import _scaffold_restatement as rs  # noqa: E402

MAX_BYTES = 720_100   # tests/golden/cases/synth3_w50/reference.json, the largest fixture before these


class Args:
    "print_scaffolds' args; `overlap` is read once at :556, once per path at :596 and once at :624"
    s, n, p, agp = pin.TARGET, 1, "out", True

    def __init__(self, overlap_gap, n_paths):
        self.overlap_gap, self._on, self._reads, self._n_paths = overlap_gap, overlap_gap is not None, 0, n_paths

    @property
    def overlap(self):
        self._reads += 1
        return self._on and 1 < self._reads <= 1 + self._n_paths


def run_print_scaffolds(mods, case, paths):
    "-> (assigned FASTA, .path text, .agp text) of the reference's print_scaffolds on `paths`; whatever it raises passes through"
    asm_mod, path_node, ntjoin_utils = mods
    nodes = []
    for path in paths:
        nodes.append([path_node.PathNode(c, o, s, e, len(dict(case["records"])[c]), "0", "0", g, g) for c, o, s, e, g, _sa, _ea in path])
        for nd, (*_, sa, ea) in zip(nodes[-1], path):
            nd.start_adjust, nd.end_adjust = sa, ea
    sc = object.__new__(asm_mod.NtjoinScaffolder)
    sc.args = Args(case["overlap_gap"], len(paths))
    sc.scaffolds = {rid: ntjoin_utils.Scaffold(id=rid, length=len(seq), sequence=seq) for rid, seq in case["records"]}
    sc.print_unassigned = lambda *a, **k: None
    sc.merge_relocations = lambda path, _incorporated: path
    cwd, tmp = os.getcwd(), tempfile.mkdtemp()
    os.chdir(tmp)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            sc.print_scaffolds(nodes, {}, collections.defaultdict(set))
        out = []
        for name in (pin.TARGET[:-4] + ".n1.assigned.scaffolds.fa", "out.path", "out.agp"):
            with open(name, encoding="ascii") as fh:
                out.append(fh.read())
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp)
    assert sc.args._reads == (len(paths) + 2 if len(paths) else 2), "print_scaffolds reads args.overlap otherwise than at :556, :596 and :624"
    return out


def record_case(mods, name, generator, gen_args):
    case = pin.GENERATORS[generator](**gen_args)
    status = []
    for path in case["paths"]:
        try:
            run_print_scaffolds(mods, case, [path])
            status.append("ok")
        except Exception as err:  # pylint: disable=broad-except
            frames = [f for f in traceback.extract_tb(err.__traceback__) if os.path.basename(f.filename) == "ntjoin_assemble.py"]
            status.append({"error": {"type": type(err).__name__, "line": frames[-1].lineno}})
    kept = [path for path, st in zip(case["paths"], status) if st == "ok"]
    assigned, path_text, agp = run_print_scaffolds(mods, case, kept)
    said = io.StringIO()
    seqs = dict(case["records"])
    for line in rs.unassigned(case["records"], kept)[0].splitlines():   # (the complement itself is bedtools' and stays unpinned)
        rid, lo, hi = line.split("\t")
        mods[0].NtjoinScaffolder.write_agp_unassigned(said, f"{rid}:{lo}-{hi}", seqs[rid][int(lo):int(hi)])
    return {"meta": {"name": name, "generator": generator, "args": gen_args, "sha256": pin.case_digest(case)}, "status": status, "path": path_text,
            "agp": agp, "agp_unassigned": said.getvalue(), "scaffolds": pin.scaffold_digests(assigned)}


def record_family(mods, family, specs):
    entries = [record_case(mods, *spec) for spec in specs]
    out = os.path.join(pin.FAMILY_DIR, family + ".json")
    with open(out, "w", encoding="ascii") as fh:
        json.dump({"meta": {"generator": "tests/golden/make_golden_scaffold_fuzz.py", "family": family, "inputs_from": "tests/_scaffold_pin.py family_specs()"},
                   "cases": entries}, fh, separators=(",", ":"))
        fh.write("\n")
    assert os.path.getsize(out) <= MAX_BYTES, (out, os.path.getsize(out))
    pin.load_family.cache_clear()
    found = pin.check_conditions(family, pin.load_family(family))   # AssertionError: a condition of the README does not hold
    print(family, len(entries), "cases,", os.path.getsize(out), "bytes;", found)


def main():
    if not os.path.isdir(mg.REF):
        sys.exit("make_golden_scaffold_fuzz.py needs the reference tree (build container only)")
    sys.path.insert(0, os.path.join(mg.REF, "bin"))
    mg.install_igraph_standin()
    asm_mod = mg.import_scaffolder()
    import ntjoin_utils
    import path_node
    os.makedirs(pin.FAMILY_DIR, exist_ok=True)
    only = sys.argv[1:]
    for family, specs in pin.family_specs().items():
        if not only or family in only:
            record_family((asm_mod, path_node, ntjoin_utils), family, specs)


if __name__ == "__main__":
    main()
