"""GPU tests of --assess on the command line (`python -m ntjoin_amd.assemble`), on the reference's own fixtures under
tests/golden/fasta at k = 32 and w = 100: <prefix>.assess.tsv and <prefix>.breakpoints.bed against the formatters over the restatement
of the contract (tests/_assess_restatement.py) over the blocks the Python API returns; every BED line inside a record of the scaffold
files; nothing else changes in a run; together with --synteny, --gz and --rounds_w; a reference given as TSV with and without its
.fai; the empty graph.  Every run is a child process under a time limit of its own."""
import glob
import os
import shutil

import pytest

from tests import _assess_restatement as A
from tests.test_gpu_assemble_synteny import EMPTY, K, RUNS, W, argv, child, fai_lengths, files, fresh
from tests.test_gpu_synteny import as_tuples

pytestmark = pytest.mark.gpu

ASSESS = ["--assess", "--synteny_min_anchors", "2"]
NEW = ("run.assess.tsv", "run.breakpoints.bed")


def restated_files(d, target, opts, monkeypatch, ref="ref.fa"):
    "the same run in-process without --assess: the formatters over the restatement over synteny_blocks' arrays -> (tsv text, bed text)"
    from ntjoin_amd import assemble
    from ntjoin_amd.ntjoin import Ntjoin
    from ntjoin_amd.report import ASSESS_COLUMNS, assess_row, breakpoint_lines
    from ntjoin_amd.run import parse_arguments, set_weights
    monkeypatch.chdir(d)
    args = parse_arguments(argv(target, *opts, ref=ref))
    fasta, w = assemble.derive_names(args)
    nj = Ntjoin(args, fasta=assemble.sources(args, fasta), w=w)
    nj.weights_list = set_weights(args)
    try:
        nj.load_minimizers_scaffold()
        nj.scaffold(keep=True)
        eng = nj._engine
        pieces, first, ids = eng.scaffold_pieces()
        rows, offs = pieces.tolist(), first.tolist()
        s_len, s_ids = eng.record_lengths(0), eng.record_ids(0, eng.n_records(0))
        blocks = eng.synteny_blocks(1, 0, max_gap=100000, min_anchors=2, min_span=0)
        whole = A.assess(as_tuples(blocks), K, eng.record_lengths(1), s_len)
        tsv = ["\t".join(ASSESS_COLUMNS), assess_row(target, ref, eng.n_records(1), blocks["n_anchors_total"], whole)]
        blocks = eng.synteny_blocks(1, 0, max_gap=100000, min_anchors=2, min_span=0, pieces=pieces, first=first)
        q_len = [sum(row[2] - row[1] for row in rows[offs[r]:offs[r + 1]]) for r in range(len(ids))]
        scaf = A.assess(as_tuples(blocks), K, q_len, s_len, pieces=rows, first=offs)
        tsv.append(assess_row(f"{target}.k{K}.w{W}.n1.all.scaffolds.fa", ref, len(ids), blocks["n_anchors_total"], scaf))
        return "\n".join(tsv) + "\n", "".join(breakpoint_lines(scaf, ids, ref, s_ids)), scaf
    finally:
        nj.close()


@pytest.mark.parametrize("ref,target", RUNS, ids=[f"{r}-{t}" for r, t in RUNS])
def test_files_of_a_run(ref, target, tmp_path, monkeypatch):
    opts = ["--overlap"]
    on, off, inproc = fresh(tmp_path, "on", target, ref), fresh(tmp_path, "off", target, ref), fresh(tmp_path, "inproc", target, ref)
    child(on, argv(target, "--fai", *opts, *ASSESS, ref=ref))
    child(off, argv(target, "--fai", *opts, ref=ref))
    before, after = files(off), files(on)
    assert not any(n in before for n in NEW) and {n: v for n, v in after.items() if n not in NEW} == before and all(n in after for n in NEW)
    tsv, bed = after[NEW[0]].decode("ascii"), after[NEW[1]].decode("ascii")
    want_tsv, want_bed, scaf = restated_files(inproc, target, opts, monkeypatch, ref)
    print(tsv, bed, sep="")   # (the rows DESIGN.md 4o quotes)
    assert tsv == want_tsv and bed == want_bed
    out = f"{target}.k{K}.w{W}.n1"
    lengths = fai_lengths(on / f"{out}.assigned.scaffolds.fa.fai", on / f"{out}.unassigned.scaffolds.fa.fai")
    ref_ids = set(fai_lengths(on / f"{ref}.fai"))
    for line in bed.splitlines():
        name, lo, hi, what, ref_name, left, right = line.split("\t")
        assert 0 <= int(lo) < int(hi) <= lengths[name] and ref_name == ref
        assert what.split("|")[0] in A.KINDS and what.split("|")[1] in ("join", "contig")
        assert left[:-1] in ref_ids and right[:-1] in ref_ids and left[-1] in "+-" and right[-1] in "+-"
    cells = [line.split("\t") for line in tsv.splitlines()]
    assert len(cells) == 3 and all(len(c) == len(cells[0]) for c in cells) and sum(int(x) for x in cells[2][-6:]) == len(bed.splitlines())
    if (ref, target) in EMPTY:   # the empty graph: rows of zeros behind the sums of lengths, NG50 apart
        for c in cells[1:]:
            assert all(x == "0" for x in c[5:19]) and all(x == "0" for x in c[21:]) and int(c[3]) > 0 and int(c[4]) > 0
        assert bed == ""
    else:
        assert scaf["n_chains"] > 0 and int(cells[2][8]) > 0


def test_with_synteny_gz_and_rounds(tmp_path):
    target = "scaf.f-r.fa"
    both, syn, alone, gz = (fresh(tmp_path, n, target) for n in ("both", "syn", "alone", "gz"))
    child(both, argv(target, "--overlap", "--synteny", *ASSESS))
    child(syn, argv(target, "--overlap", "--synteny", "--synteny_min_anchors", "2"))
    child(alone, argv(target, "--overlap", *ASSESS))
    child(gz, argv(target, "--overlap", "--gz", *ASSESS))
    a, b, c, z = files(both), files(syn), files(alone), files(gz)
    assert {n: v for n, v in a.items() if n not in NEW} == b and {n: v for n, v in a.items() if n != "run.synteny.paf"} == c
    assert a["run.synteny.paf"] and a[NEW[0]].count(b"\n") == 3
    assert z[NEW[0]] == c[NEW[0]].replace(b".all.scaffolds.fa\t", b".all.scaffolds.fa.gz\t") and z[NEW[1]] == c[NEW[1]]
    rounds = fresh(tmp_path, "rounds", target)
    child(rounds, argv(target, "--overlap", "--rounds_w", "50", *ASSESS))
    assert sorted(os.path.basename(p) for p in glob.glob(str(rounds / "run*.assess.tsv")) + glob.glob(str(rounds / "run*.breakpoints.bed"))) == \
        ["run.round2.assess.tsv", "run.round2.breakpoints.bed"]
    last = (rounds / "run.round2.assess.tsv").read_text().splitlines()
    assert len(last) == 3 and last[1].split("\t")[0] == f"{target}.k{K}.w{W}.n1.all.scaffolds.fa"
    assert last[2].split("\t")[0] == f"{target}.k{K}.w{W}.n1.all.scaffolds.fa.k{K}.w50.n1.all.scaffolds.fa"


def test_reference_given_as_tsv(tmp_path):
    "no lengths in the handle: left out with one line on stderr without <fasta>.fai, used with it"
    target = "scaf.f-f.fa"
    d = fresh(tmp_path, "d", target)
    first = child(d, argv(target, "--fai", *ASSESS))   # sketches the reference, leaves its TSV and its .fai
    assert "has no .fai" not in first.stderr
    want = [(d / n).read_bytes() for n in NEW]
    assert want[0].count(b"\n") == 3
    shutil.move(d / "ref.fa.fai", d / "kept.fai")
    second = child(d, argv(target, *ASSESS))
    assert f"ntjoin_amd: ref.fa.k{K}.w{W}.tsv was loaded from its TSV and its FASTA has no .fai: the assessment has no rows for it" in second.stderr
    assert (d / NEW[0]).read_bytes().count(b"\n") == 1 and (d / NEW[1]).read_bytes() == b""
    shutil.move(d / "kept.fai", d / "ref.fa.fai")
    third = child(d, argv(target, *ASSESS))
    assert "has no .fai" not in third.stderr and [(d / n).read_bytes() for n in NEW] == want
