#!/usr/bin/env python3
"""Goldens of the path adjustment stage (tests/golden/adjust/*.json).  BUILD CONTAINER ONLY, like its siblings: it reads the
reference tree, and it only imports it.

The reference's OWN functions run in main_scaffolder's order (bin/ntjoin_assemble.py:775-784 and the head of print_scaffolds
:549-553) on PathNodes made from recorded or hand-made rows: tally_incorporated_segments and merge_relocations (as
format_adjust_paths calls them), adjust_paths with no_cut, tally_intersecting_segments (OverlapRegion.find_non_overlapping behind
it; pybedtools_standin.py for the sort and the intersection counts), then merge_relocations, remove_overlapping_regions and
check_terminal_node_gap_zero per path.  Recorded per case: the input rows, no_cut and G, the resulting rows, and per resulting
node the (path, node) of the input row it is.

Cases: the format_by_n rows of four fixtures under tests/golden/cases (regions-ff-rr at n = 1 with and without no_cut,
regions-fr-rf at n = 2, gap-dist and f-f-f at n = 1) and the hand-made cases of tests/_adjust_cases.py.

Families (tests/golden/adjust/families/<family>.json): the seeded inputs of tests/_adjust_cases.py family_specs() (fuzz, ladder,
strided, large).  Their inputs are not written: a case holds its generator's arguments and the sha256 of the input, its result
and source packed against that input without loss (_adjust_cases.pack_result; for the large case their digests, the node counts
and the first paths), or the KeyError the reference raised as
{"error": {"path", "contig", "start", "end"}}: the path whose merge_relocations call raised and the Bed that was not in the set.
Every case runs under both orders of equal starts (pybedtools_standin.py); meta.tie_independent says whether the two agree, and
the recorded answer is the one under the project's rule (the smaller end first)."""
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import pybedtools_standin  # noqa: E402
from tests import _adjust_cases  # noqa: E402

OUT = os.path.join(HERE, "adjust")
FIXTURES = [("regions-ff-rr_n1", "regions-ff-rr_w500", "1", False), ("regions-ff-rr_n1_no_cut", "regions-ff-rr_w500", "1", True),
            ("regions-fr-rf_n2", "regions-fr-rf_w500", "2", False), ("gap-dist_n1", "gap-dist_w500", "1", False),
            ("f-f-f_n1", "f-f-f_w1000", "1", False)]


def run_reference(asm_mod, path_node, ntjoin_utils, rows, no_cut, G):
    paths = []
    for p, path in enumerate(rows):
        nodes = [path_node.PathNode(*row) for row in path]
        for i, node in enumerate(nodes):
            node.where = [p, i]
        paths.append(nodes)
    sc = object.__new__(asm_mod.NtjoinScaffolder)
    sc.args = types.SimpleNamespace(G=G, no_cut=no_cut)
    scaffolds = {node.contig: ntjoin_utils.Scaffold(id=node.contig, length=node.contig_size, sequence="") for path in paths for node in path}
    segments = {}
    for path in paths:  # format_adjust_paths :704-719
        sc.tally_incorporated_segments(segments, path)
    paths = [sc.merge_relocations(path, segments) for path in paths]
    if no_cut:
        paths = sc.adjust_paths(paths, scaffolds, segments)
    fixes = sc.tally_intersecting_segments(segments)
    for i, path in enumerate(paths):  # print_scaffolds :549-553
        new_path = sc.merge_relocations(path, segments)
        new_path = sc.remove_overlapping_regions(new_path, fixes)
        sc.check_terminal_node_gap_zero(new_path)
        paths[i] = new_path
    result = [[[nd.contig, nd.ori, nd.start, nd.end, nd.contig_size, nd.first_mx, nd.terminal_mx, nd.gap_size, nd.raw_gap_size] for nd in path]
              for path in paths]
    return result, [[nd.where for nd in path] for path in paths]


def run_family_case(asm_mod, path_node, ntjoin_utils, case):
    "-> {'result', 'source'} or {'error'}: run_reference, with the per-path merge_relocations calls wrapped to learn which path raised"
    plain, raised = asm_mod.NtjoinScaffolder.merge_relocations, []

    def wrapped(self, path, incorporated_segments):
        try:
            return plain(self, path, incorporated_segments)
        except KeyError:
            raised.append(path[0].where[0])
            raise

    asm_mod.NtjoinScaffolder.merge_relocations = wrapped
    try:
        result, source = run_reference(asm_mod, path_node, ntjoin_utils, json.loads(json.dumps(case["paths"])), case["no_cut"], case["G"])
    except KeyError as err:
        bed = err.args[0]
        return {"error": {"path": raised[0], "contig": bed.contig, "start": bed.start, "end": bed.end}}
    finally:
        asm_mod.NtjoinScaffolder.merge_relocations = plain
    return {"result": result, "source": source}


def record_families(asm_mod, path_node, ntjoin_utils):
    os.makedirs(os.path.join(OUT, "families"), exist_ok=True)
    for family, specs in _adjust_cases.family_specs().items():
        entries, tied = [], []
        for name, generator, args in specs:
            case = _adjust_cases.check_case(_adjust_cases.GENERATORS[generator](**args))
            answers = []
            for larger_end_first in (False, True):
                pybedtools_standin.EQUAL_START_LARGER_END_FIRST = larger_end_first
                try:
                    answers.append(run_family_case(asm_mod, path_node, ntjoin_utils, case))
                finally:
                    pybedtools_standin.EQUAL_START_LARGER_END_FIRST = False
            answer = answers[0]
            if family == "large":
                answer = _adjust_cases.summarise_large(answer["result"], answer["source"])
            elif "error" not in answer:
                answer = {"nodes": _adjust_cases.pack_result(case, answer["result"], answer["source"])}
            if answers[0] != answers[1]:
                tied.append(name)
            entries.append({"meta": {"name": name, "generator": generator, "args": args, "sha256": _adjust_cases.case_digest(case),
                                     "tie_independent": answers[0] == answers[1]}, **answer})
        doc = {"meta": {"generator": "tests/golden/make_golden_adjust.py", "family": family,
                        "inputs_from": "tests/_adjust_cases.py family_specs()"}, "cases": entries}
        path = os.path.join(OUT, "families", family + ".json")
        with open(path, "w", encoding="ascii") as fh:
            json.dump(doc, fh, separators=(",", ":"))
            fh.write("\n")
        print(family, len(entries), "cases,", sum("error" in e for e in entries), "errors,", len(tied), "tie-dependent", tied, os.path.getsize(path), "bytes")


def main():
    if not os.path.isdir(mg.REF):
        sys.exit("make_golden_adjust.py needs the reference tree (build container only)")
    sys.path.insert(0, os.path.join(mg.REF, "bin"))
    mg.install_igraph_standin()
    sys.modules["pybedtools"] = pybedtools_standin
    asm_mod = mg.import_scaffolder()
    import ntjoin_utils
    import path_node
    os.makedirs(OUT, exist_ok=True)

    def record(name, rows, no_cut, G, origin):
        result, source = run_reference(asm_mod, path_node, ntjoin_utils, json.loads(json.dumps(rows)), no_cut, G)
        doc = {"meta": {"generator": "tests/golden/make_golden_adjust.py", "paths_from": origin}, "no_cut": no_cut, "G": G, "paths": rows,
               "result": result, "source": source}
        with open(os.path.join(OUT, name + ".json"), "w", encoding="ascii") as fh:
            json.dump(doc, fh, separators=(",", ":"))
            fh.write("\n")
        print(name, sum(map(len, rows)), "->", sum(map(len, result)), "nodes")

    for name, case, n, no_cut in FIXTURES:
        with open(os.path.join(HERE, "cases", case, "reference.json"), encoding="utf-8") as fh:
            ref = json.load(fh)["reference"]
        record(name, ref["format_by_n"][n], no_cut, int(ref["format_args"].get("G", 0)),
               f"format_path as recorded in tests/golden/cases/{case} (n={n})")
    for name, case in _adjust_cases.hand_cases().items():
        record("hand_" + name, case["paths"], case["no_cut"], case["G"], "tests/_adjust_cases.py hand_cases()")
    record_families(asm_mod, path_node, ntjoin_utils)


if __name__ == "__main__":
    main()
