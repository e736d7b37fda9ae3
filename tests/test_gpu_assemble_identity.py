"""GPU tests of --identity on the command line (`python -m ntjoin_amd.assemble`), on the reference's own fixtures under
tests/golden/fasta at k = 32 and w = 100: <prefix>.identity.tsv and the identity tags of <prefix>.synteny.paf against the restatement
of the contract (tests/_identity_restatement.py: a plain DP) over the graph arrays read through the Python API, the written scaffold
FASTA and the reference FASTA; nothing else changes in a run, and a run without --identity leaves exactly the files it left before;
together with --synteny, --assess, --gz and --rounds_w; a reference given as TSV.  Every run is a child process under a time limit
of its own."""
import glob
import os

import pytest

from tests import _identity_restatement as R, _synteny_restatement as SR
from tests.test_gpu_assemble_synteny import EMPTY, FASTA, K, RUNS, W, argv, child, files, fresh, read_fasta

pytestmark = pytest.mark.gpu

IDENTITY = ["--identity", "--synteny_min_anchors", "2"]
NEW = "run.identity.tsv"
COLUMNS = ("query reference blocks segments aligned skipped_len skipped_shift skipped_n saturated block_query_bases aligned_query "
           "aligned_subject edits edits_per_100kbp").split()


def row(query, reference, res):
    cells = [query, reference] + [res[n] for n in ("n_blocks", "n_segments", "n_aligned", "n_skip_len", "n_skip_shift", "n_skip_n", "n_saturated",
                                                   "block_q", "aligned_q", "aligned_s", "edits")]
    return "\t".join(str(c) for c in cells) + "\t" + R.per_100kbp(res["edits"], res["aligned_q"], res["aligned_s"])


def restated(d, on, target, opts, monkeypatch, ref="ref.fa", max_seg=10000, ext=".fa"):
    """the same run in-process without --identity, for the graph arrays and the piece table; the bases come from the FASTA files: the
    reference's and the target's as they lie under tests/golden, the scaffolds' as the run under test wrote them
    -> (the identity table's text, the restatement of the scaffolds' blocks, the scaffolds' PAF without tags)"""
    from ntjoin_amd import assemble
    from ntjoin_amd.ntjoin import Ntjoin
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
        g = eng.get_graph()
        pieces, first, ids = eng.scaffold_pieces()
        rows, offs = pieces.tolist(), first.tolist()
        ref_ids, tgt_ids = eng.record_ids(0, eng.n_records(0)), eng.record_ids(1, eng.n_records(1))
        eng.synteny_blocks(1, 0, max_gap=100000, min_anchors=2, min_span=0, pieces=pieces, first=first)
        eng.write_synteny_paf("plain.paf", query_names=ids)   # (the 13 columns, as --synteny writes them)
        with open("plain.paf", "rb") as fh:
            plain = fh.read()
    finally:
        nj.close()
    ref_seq, tgt_seq = read_fasta(os.path.join(FASTA, ref)), read_fasta(os.path.join(FASTA, target))
    out = f"{target}.k{K}.w{W}.n1"
    scaf_seq = dict(read_fasta(on / f"{out}.assigned.scaffolds{ext}"), **read_fasta(on / f"{out}.unassigned.scaffolds{ext}"))
    kw = dict(max_gap=100000, min_anchors=2, min_span=0, max_seg=max_seg)
    whole = R.synteny_identity(SR.anchor_list(g["vertex_pos"], g["vertex_record"], 1, 0, K), K, [tgt_seq[i] for i in tgt_ids],
                               [ref_seq[i] for i in ref_ids], **kw)
    scaf = R.synteny_identity(SR.anchor_list(g["vertex_pos"], g["vertex_record"], 1, 0, K, rows, offs), K, [scaf_seq[i] for i in ids],
                              [ref_seq[i] for i in ref_ids], **kw)
    text = "\n".join(["\t".join(COLUMNS), row(target, ref, whole), row(f"{out}.all.scaffolds{ext}", ref, scaf)]) + "\n"
    return text, scaf, plain


def tagged(plain_paf, scaf):
    lines = plain_paf.decode("ascii").splitlines()
    b = scaf["blocks"]
    assert len(lines) == scaf["n_blocks"]
    return "".join(line + R.paf_tags(b["aligned_q"][i], b["aligned_s"][i], b["edits"][i]) + "\n" for i, line in enumerate(lines)).encode("ascii")


@pytest.mark.parametrize("ref,target", RUNS, ids=[f"{r}-{t}" for r, t in RUNS])
def test_files_of_a_run(ref, target, tmp_path, monkeypatch):
    opts = ["--overlap"]
    on, off, inproc = (fresh(tmp_path, n, target, ref) for n in ("on", "off", "inproc"))
    child(on, argv(target, *opts, "--synteny", *IDENTITY, ref=ref))
    child(off, argv(target, *opts, ref=ref))
    before, tags = files(off), files(on)
    # nothing else changes; the PAF's first 13 columns are those of a run without --identity
    assert NEW not in before and {n: v for n, v in tags.items() if n not in (NEW, "run.synteny.paf")} == before
    want, scaf, plain = restated(inproc, on, target, opts, monkeypatch, ref)
    tsv = tags[NEW].decode("ascii")
    print(tsv, end="")   # (the rows DESIGN.md 4p quotes)
    assert tsv == want
    assert tags["run.synteny.paf"] == tagged(plain, scaf)
    cells = [line.split("\t") for line in tsv.splitlines()]
    assert len(cells) == 3 and all(len(c) == len(COLUMNS) for c in cells)
    if (ref, target) in EMPTY:
        assert all(x == "0" for c in cells[1:] for x in c[2:13]) and cells[1][13] == cells[2][13] == "0.00" and tags["run.synteny.paf"] == b""
    else:
        assert int(cells[1][4]) > 0 and int(cells[2][4]) > 0 and int(cells[2][10]) > 0 and b"\tal:i:" in tags["run.synteny.paf"]
        assert all(int(c[3]) == sum(int(x) for x in c[4:8]) for c in cells[1:])


def test_with_assess_gz_max_seg_and_rounds(tmp_path, monkeypatch):
    target = "scaf.f-r.fa"
    alone, asz, both, gz, small, inproc, off, syn = (fresh(tmp_path, n, target) for n in ("alone", "asz", "both", "gz", "small", "inproc", "off", "syn"))
    child(alone, argv(target, "--overlap", *IDENTITY))
    child(off, argv(target, "--overlap"))
    child(syn, argv(target, "--overlap", "--synteny", "--synteny_min_anchors", "2"))
    child(asz, argv(target, "--overlap", "--assess", "--synteny_min_anchors", "2"))
    child(both, argv(target, "--overlap", "--assess", "--synteny", *IDENTITY))
    child(gz, argv(target, "--overlap", "--gz", *IDENTITY))
    child(small, argv(target, "--overlap", "--identity_max_seg", "60", *IDENTITY))
    a, b, c, z, s = files(alone), files(asz), files(both), files(gz), files(small)
    assert {n: v for n, v in a.items() if n != NEW} == files(off)   # identity alone: one file more
    plain = files(syn)["run.synteny.paf"]
    assert [ln.split(b"\tal:i:")[0] for ln in c["run.synteny.paf"].splitlines()] == plain.splitlines() and plain
    assert {n: v for n, v in c.items() if n not in (NEW, "run.synteny.paf")} == b and c[NEW] == a[NEW] and b"\tNM:i:" in c["run.synteny.paf"]
    assert z[NEW] == a[NEW].replace(b".all.scaffolds.fa\t", b".all.scaffolds.fa.gz\t")
    want, _, _ = restated(inproc, gz, target, ["--overlap", "--gz"], monkeypatch, ext=".fa.gz")
    assert z[NEW].decode("ascii") == want
    inproc2 = fresh(tmp_path, "inproc2", target)
    want, _, _ = restated(inproc2, small, target, ["--overlap"], monkeypatch, max_seg=60)
    assert s[NEW].decode("ascii") == want and s[NEW] != a[NEW] and int(want.splitlines()[2].split("\t")[5]) > 0
    rounds = fresh(tmp_path, "rounds", target)
    child(rounds, argv(target, "--overlap", "--rounds_w", "50", *IDENTITY))
    assert [os.path.basename(p) for p in glob.glob(str(rounds / "run*.identity.tsv"))] == ["run.round2.identity.tsv"]
    last = (rounds / "run.round2.identity.tsv").read_text().splitlines()
    assert len(last) == 3 and last[1].split("\t")[0] == f"{target}.k{K}.w{W}.n1.all.scaffolds.fa"


def test_reference_given_as_tsv(tmp_path):
    "the handle holds no text of a reference that came as its TSV: one line on stderr and no rows; the PAF lines carry no tags"
    target = "scaf.f-f.fa"
    d = fresh(tmp_path, "d", target)
    first = child(d, argv(target, "--fai", "--synteny", *IDENTITY))   # sketches the reference, leaves its TSV and its .fai
    assert "identity table" not in first.stderr and (d / NEW).read_bytes().count(b"\n") == 3
    tags = (d / "run.synteny.paf").read_bytes()
    second = child(d, argv(target, "--synteny", *IDENTITY))
    assert f"ntjoin_amd: ref.fa.k{K}.w{W}.tsv was loaded from its TSV and the handle holds no text of it: the identity table has no rows for it" \
        in second.stderr
    assert (d / NEW).read_bytes() == ("\t".join(COLUMNS) + "\n").encode()
    plain = (d / "run.synteny.paf").read_bytes()
    assert plain and b"al:i:" not in plain and [ln.split(b"\tal:i:")[0] for ln in tags.splitlines()] == plain.splitlines()
