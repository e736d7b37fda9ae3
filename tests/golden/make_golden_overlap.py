#!/usr/bin/env python3
"""Goldens of the overlap stage's cut points (tests/golden/overlap/*.json).  BUILD CONTAINER ONLY, like make_golden.py: the only
thing here that reads the reference tree, and it only imports it.

The reference's OWN adjust_for_trimming / tally_minimizers_overlap (bin/ntjoin_assemble.py:468-516) and merge_overlapping_path /
merge_overlapping (bin/ntjoin_overlap.py) run on a segments file written the way print_scaffolds writes it (:556-576), with
tests/golden/igraph_standin.py for python-igraph and a `btllib` stand-in whose Indexlr yields the C oracle's sketch of that
file.  Recorded: the nodes and, per node, start_adjust, end_adjust and whether merge_overlapping reported a cut for the
junction behind the node.

Cases:
  * the reference's three overlap fixtures, nodes from its own format_path at k = 32, w = 1000, n = 2 (weights 2 / 1),
    cuts at its defaults overlap_k = 15, overlap_w = 10;
  * a synthetic set (tests/_overlap_cases.py make_synth: contigs and paths are a function of the seed and are not committed,
    only their digest and the reference's answers are): every contig is used by one node, so that the file walk of
    adjust_for_trimming, which matches sketch records to paths by id, is the per-path contract.
"""
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
from tests import _oracle, _overlap_cases as cases, _overlap_restatement as rs  # noqa: E402

OUT = os.path.join(HERE, "overlap")
FASTA = os.path.join(HERE, "fasta")


def install_btllib_standin(orc, variant=_oracle.V2_SUM):
    mod = types.ModuleType("btllib")

    class IndexlrFlag:
        LONG_MODE = 0

    class Indexlr:
        def __init__(self, path, k, w, flags, threads):
            self.path, self.k, self.w = path, k, w

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

        def __iter__(self):
            for rid, seq in _oracle.read_fasta(self.path):
                mxs = [types.SimpleNamespace(out_hash=h, pos=p) for h, p, _f, _m in orc.sketch(seq, self.k, self.w, variant)]
                yield types.SimpleNamespace(id=rid, minimizers=mxs)

    mod.Indexlr, mod.IndexlrFlag = Indexlr, IndexlrFlag
    sys.modules["btllib"] = mod


def reference_cuts(asm_mod, paths, seqs, k, w):
    """paths: lists of the reference's PathNode -> per path (start_adjust, end_adjust, cut_found)"""
    import ntjoin_overlap
    import path_node  # noqa: F401
    orig = ntjoin_overlap.merge_overlapping

    def recording(list_mxs, list_mx_info, source, target, nodes):
        res = orig(list_mxs, list_mx_info, source, target, nodes)
        nodes[source].cut_found = bool(res)
        return res

    ntjoin_overlap.merge_overlapping = recording
    tmp = tempfile.mkdtemp()
    try:
        seg = os.path.join(tmp, "p.segments.fa")
        with open(seg, "w", encoding="ascii") as fh:  # print_scaffolds :559-575
            for nodes in paths:  # one record per node: id contig_start_end, the text of the contract
                lens = [n.end - n.start for n in nodes]
                masks = rs.mask_coords(lens, [n.raw_gap_size for n in nodes], k, w)
                for node, (l, r) in zip(nodes, masks):
                    text = rs.segment_text(seqs[node.contig], node.ori, node.start, node.end)
                    fh.write(f">{node.contig}_{node.start}_{node.end}\n{text[:l]}{'N' * (r - l)}{text[r:]}\n")
        sc = object.__new__(asm_mod.NtjoinScaffolder)
        sc.args = types.SimpleNamespace(overlap_k=k, overlap_w=w, btllib_t=1)
        with contextlib.redirect_stdout(io.StringIO()):
            sc.adjust_for_trimming(seg, paths)
    finally:
        ntjoin_overlap.merge_overlapping = orig
        shutil.rmtree(tmp)
    return [([n.start_adjust for n in nodes], [n.end_adjust for n in nodes], [bool(getattr(n, "cut_found", False)) for n in nodes])
            for nodes in paths]


def stats_of(paths, kinds):
    st = {"junctions": 0, "overlapping": 0, "cut": 0, "run": 0, "single": 0, "none": 0, "even_run_string_order": 0, "pairs": set()}
    for nodes, kd in zip(paths, kinds):
        for i in range(len(nodes) - 1):
            st["junctions"] += 1
            st["pairs"].add(nodes[i][1] + nodes[i + 1][1])
            if nodes[i][4] < 0:
                st["overlapping"] += 1
                kind, n, differs = kd[i]
                st[kind] += 1
                st["cut"] += kind != "none"
                st["even_run_string_order"] += kind == "run" and n % 2 == 0 and differs
    st["pairs"] = sorted(st["pairs"])
    return st


def check_stats(st):
    assert st["junctions"] >= 200 and len(st["pairs"]) == 4, st
    assert 2 * st["cut"] >= st["overlapping"], st
    assert min(st["run"], st["single"], st["none"], st["even_run_string_order"]) >= 10, st


def main():
    if not os.path.isdir(mg.REF):
        sys.exit("make_golden_overlap.py needs the reference tree (build container only)")
    _oracle.build()
    orc = _oracle.load()
    mg.install_igraph_standin()
    sys.path.insert(0, os.path.join(mg.REF, "bin"))
    install_btllib_standin(orc)
    asm_mod = mg.import_scaffolder()
    import path_node
    os.makedirs(OUT, exist_ok=True)

    def sketch(text, k, w):
        return [(h, p) for h, p, _f, _m in orc.sketch(text, k, w)]

    def record(name, fasta, paths9, seqs, k, w, extra):
        nodes = [[path_node.PathNode(*nd) for nd in path] for path in paths9]
        got = reference_cuts(asm_mod, nodes, seqs, k, w)
        mine = rs.cuts([[(nd[0], nd[1], nd[2], nd[3], nd[8]) for nd in path] for path in paths9], seqs, k, w, sketch)
        assert [list(g[0]) for g in got] == mine[0] and [list(g[1]) for g in got] == mine[1] and [list(g[2]) for g in got] == mine[2], \
            f"{name}: the restatement disagrees with the reference"
        doc = {"meta": {"generator": "tests/golden/make_golden_overlap.py", "k": k, "w": w, "variant": "v2", "fasta": fasta},
               "paths": paths9, "start_adjust": [g[0] for g in got], "end_adjust": [g[1] for g in got],
               "cut_found": [g[2] for g in got]}
        doc["meta"].update(extra)
        if "synth" in extra:  # inputs are re-made from the seed
            del doc["paths"], doc["meta"]["fasta"]
            for key in ("start_adjust", "end_adjust"):
                doc[key] = [list(v) for v in doc[key]]
            doc["cut_found"] = [[int(c) for c in v] for v in doc["cut_found"]]
        with open(os.path.join(OUT, name + ".json"), "w", encoding="ascii") as fh:
            json.dump(doc, fh, separators=(",", ":"))
            fh.write("\n")
        return mine[3]

    # ---- the reference's fixtures
    expected = {"scaf.f-f.overlapping.fa": "1+:0-2033 20N 2+:34-2331", "scaf.f-r.overlapping.fa": "1+:0-2033 20N 2-:0-2297",
                "scaf.r-r.overlapping.fa": "1-:66-2099 20N 2-:0-2297"}
    for fa, want in expected.items():
        src = os.path.join(mg.REF, "tests", fa)
        dst = os.path.join(FASTA, fa)
        if not os.path.exists(dst):
            shutil.copyfile(src, dst)  # a data file of the reference's tests
        tmp = tempfile.mkdtemp()
        try:
            tsvs = []
            for f in ("ref.fa", fa):
                shutil.copyfile(os.path.join(FASTA, f), os.path.join(tmp, f))
                tsvs.append(f + ".k32.w1000.tsv")
                orc.fasta_to_tsv(os.path.join(tmp, f), os.path.join(tmp, tsvs[-1]), 32, 1000)
            ref = mg.run_reference(tmp, [tsvs[0]], [2], tsvs[1], 1, "out", k=32, target_fasta=os.path.join(tmp, fa))
        finally:
            shutil.rmtree(tmp)
        paths9 = [[nd for nd in path if nd[1] != "?"] for path in ref["format_by_n"]["2"]]
        paths9 = [p for p in paths9 if len(p) >= 2]
        for p in paths9:  # check_terminal_node_gap_zero (:441-448)
            p[-1][7] = 0
        record(fa.replace("scaf.", "").replace(".fa", ""), fa, paths9, dict(_oracle.read_fasta(dst)), 15, 10,
               {"reference_path": want, "paths_from": "format_path at k=32 w=1000 n=2, weights 2/1"})

    # ---- the synthetic set
    seed, n_paths = 20261016, 40
    records, paths = cases.make_synth(seed, n_paths)
    seqs = dict(records)
    syn = {"seed": seed, "n_paths": n_paths, "sha256": cases.digest(records, paths)}
    for k, w in ((15, 10), (32, 64)):
        kinds = record(f"synth_k{k}_w{w}", None, cases.paths9(records, paths), seqs, k, w, {"synth": syn})
        st = stats_of(paths, kinds)
        print(f"synth k={k} w={w}:", st)
        if (k, w) == (15, 10):
            check_stats(st)

if __name__ == "__main__":
    main()
