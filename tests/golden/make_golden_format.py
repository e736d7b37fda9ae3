#!/usr/bin/env python3
"""Goldens of the path stage on generated inputs (tests/golden/format/families/<family>.json).  BUILD CONTAINER ONLY, like its
siblings: it reads the reference tree, and it only imports it.

Per case of tests/_format_cases.py family_specs() (fuzz, m_rule, gaps, wide) the assemblies are written as minimizer TSVs into a
temporary directory and the reference's OWN functions run on them in make_golden.run_reference's order: Ntjoin.load_minimizers,
read_minimizers for the target, make_minimizer_graph, filter_graph_global, find_paths; then, on an NtjoinScaffolder made with
object.__new__ that holds args (k, g, G, m, mkt=False, s), list_mx_info, the filtered graph and the scaffolds' lengths,
find_mx_min_max and format_path(path, target, sub) for every path.  Every case runs without --mkt (pymannkendall is not here).

Recorded per case: meta (the generator's name and arguments, the sha256 of the input, for the hand-made cases their tags and the
line of arithmetic), the paths as lists of indexes into the case's ascending hashes, in ascending order of those lists, and per
path the nine-column rows, hashes as such indexes too; where format_path raised ValueError, null for the path's rows and
{"error": {"path", "u", "v"}} from the message the reference printed.  The wide case holds the digests of its paths and rows, the
node count per path and the first paths verbatim.  The inputs are not written: tests/_format_cases.py load_family() re-makes them.
The conditions of tests/golden/format/README.md are asserted on what was recorded; a failure leaves the script with a non-zero
status."""
import contextlib
import io
import json
import os
import re
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from tests import _format_cases as fc  # noqa: E402

OUT = os.path.join(HERE, "format")


def run_reference(asm_mod, ntjoin, ntjoin_utils, case):
    "-> (paths as lists of hash strings, rows per path or None where format_path raised, [(path, u contig, v contig)] of the raises)"
    with tempfile.TemporaryDirectory() as tmp:
        fc.write_tsvs(case, tmp)
        names = [name + ".tsv" for name in fc.asm_names(case)]
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            args = types.SimpleNamespace(p="out", FILES=names[:-1], t=1, s=names[-1], l=float(case["weights"][-1]), n=case["n"])
            nj = ntjoin.Ntjoin(args)
            nj.weights_list = [float(w) for w in case["weights"][:-1]]
            with contextlib.redirect_stdout(io.StringIO()):
                nj.load_minimizers()
                info, mxs = ntjoin_utils.read_minimizers(args.s)
                nj.list_mx_info[args.s], nj.list_mxs[args.s], nj.weights[args.s] = info, mxs, args.l
                nj.make_minimizer_graph()
                nj.graph = nj.filter_graph_global(nj.graph)
                found = nj.find_paths()
        finally:
            os.chdir(cwd)
    sc = object.__new__(asm_mod.NtjoinScaffolder)
    sc.args = types.SimpleNamespace(k=case["k"], g=case["g"], G=case["G"], m=case["m"], mkt=False, s=args.s)
    sc.list_mx_info, sc.graph = nj.list_mx_info, nj.graph
    sc.scaffolds = {c: ntjoin_utils.Scaffold(id=c, length=n, sequence="") for c, n in case["lengths"].items()}
    sc.mx_extremes = sc.find_mx_min_max(args.s)
    paths, rows, raised = [], [], []
    for comp in found:
        for path, sub in comp:
            said = io.StringIO()
            try:
                with contextlib.redirect_stdout(said):
                    nodes = sc.format_path(path, args.s, sub)
                nodes = [[nd.contig, nd.ori, nd.start, nd.end, nd.contig_size, nd.first_mx, nd.terminal_mx, nd.gap_size, nd.raw_gap_size] for nd in nodes]
            except ValueError:
                u, v = re.findall(r"^Contig:(\S+)\t", said.getvalue(), flags=re.M)
                assert "Gap distance estimation less than 0" in said.getvalue()
                nodes = None
                raised.append((list(path), u, v))
            paths.append(list(path))
            rows.append(nodes)
    return paths, rows, raised


def record_family(asm_mod, ntjoin, ntjoin_utils, family, specs):
    entries = []
    for name, generator, gen_args in specs:
        case = fc.GENERATORS[generator](**gen_args)
        paths, rows, raised = run_reference(asm_mod, ntjoin, ntjoin_utils, case)
        index = {str(h): i for i, h in enumerate(fc.universe(case))}
        paths, rows = fc.pack(case, paths, rows)
        meta = {"name": name, "generator": generator, "args": gen_args, "sha256": fc.case_digest(case)}
        if "tags" in case:
            meta["tags"], meta["doc"] = case["tags"], case["doc"]
        entry = {"meta": meta}
        if raised:
            assert len(raised) == 1, (name, raised)
            path, u, v = raised[0]
            entry["error"] = {"path": paths.index([index[x] for x in path]), "u": u, "v": v}
        if family == "wide":
            assert not raised
            entry.update(fc.summarise_wide(paths, rows))
        else:
            entry.update(paths=paths, rows=rows)
        entries.append(entry)
    doc = {"meta": {"generator": "tests/golden/make_golden_format.py", "family": family, "inputs_from": "tests/_format_cases.py family_specs()"},
           "cases": entries}
    path = os.path.join(OUT, "families", family + ".json")
    with open(path, "w", encoding="ascii") as fh:
        json.dump(doc, fh, separators=(",", ":"))
        fh.write("\n")
    assert os.path.getsize(path) < 200_000, (path, os.path.getsize(path))
    fc.load_family.cache_clear()
    found = fc.check_conditions(family, fc.load_family(family))   # AssertionError: a condition of the README does not hold
    print(family, len(entries), "cases,", sum("error" in e for e in entries), "errors,", os.path.getsize(path), "bytes;",
          found if family in ("fuzz", "wide") else "")


def main():
    if not os.path.isdir(mg.REF):
        sys.exit("make_golden_format.py needs the reference tree (build container only)")
    sys.path.insert(0, os.path.join(mg.REF, "bin"))
    mg.install_igraph_standin()
    asm_mod = mg.import_scaffolder()
    import ntjoin
    import ntjoin_utils
    os.makedirs(os.path.join(OUT, "families"), exist_ok=True)
    only = sys.argv[1:]
    for family, specs in fc.family_specs().items():
        if not only or family in only:
            record_family(asm_mod, ntjoin, ntjoin_utils, family, specs)


if __name__ == "__main__":
    main()
