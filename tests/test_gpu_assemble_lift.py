"""GPU tests of --lift on the command line (`python -m ntjoin_amd.assemble`), through the make front-end and with --rounds_w, on the
reference's own fixtures under tests/golden/fasta at k = 32 and w = 100: the misassembled target against the reference it was made
from, so that a contig is cut and a piece is reverse-complemented.  The BED file is made from the run's own piece table: features on
both sides of a cut, across it, on a reverse piece, on what no scaffold holds, on an unknown contig.  The lifted and unlifted files
equal the restatement of the contract (tests/_lift_restatement.py) applied to scaffold_pieces() -- with --rounds_w to the table that
<p>.rounds.agp spells -- and every lifted interval, read back from the scaffold FASTA, spells the feature's bases of the target
FASTA, reverse-complemented under a flipped strand.  Every run is a child process under a time limit of its own."""
import os
import subprocess
import sys

import pytest

from tests import _compose_restatement as C, _lift_restatement as R
from tests.conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu

FASTA = os.path.join(GOLDEN, "fasta")
ENV = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
LIMIT = ["timeout", "-k", "10", "120"]
K, W = 32, 100
TARGET, REF = "scaf.misassembled.f-r.r-f.fa", "ref.multiple.fa"
OUT = f"{TARGET}.k{K}.w{W}.n1"


def argv(*opts):
    # (--lift's list of files ends at the next option)
    return list(opts) + ["-p", "run", "-n", "1", "-s", f"{TARGET}.k{K}.w{W}.tsv", "-l", "1", "-r", "2", "-k", str(K), f"{REF}.k{K}.w{W}.tsv"]


def child(cwd, words):
    res = subprocess.run(LIMIT + words, cwd=cwd, env=ENV, capture_output=True, text=True, check=False)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    return res


def fresh(tmp_path, name):
    d = tmp_path / name
    d.mkdir()
    for fa in (TARGET, REF):
        os.symlink(os.path.join(FASTA, fa), d / fa)
    return d


def read_fasta(path):
    seqs, name = {}, None
    with open(path, "rt") as fh:
        for line in fh:
            if line.startswith(">"):
                name = line[1:].split()[0]
                assert name not in seqs
                seqs[name] = []
            else:
                seqs[name].append(line.strip())
    return {n: "".join(parts) for n, parts in seqs.items()}


def rc(s):
    return s[::-1].translate(C.COMP)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """the run in-process, without --lift: the scaffolds' piece table as the Python API hands it out, the target's records, and a
    BED file made from them -> dict"""
    from ntjoin_amd import assemble
    from ntjoin_amd.ntjoin import Ntjoin
    from ntjoin_amd.run import parse_arguments, set_weights
    d = fresh(tmp_path_factory.mktemp("lift"), "inproc")
    cwd = os.getcwd()
    os.chdir(d)
    try:
        args = parse_arguments(argv())
        fasta, w = assemble.derive_names(args)
        nj = Ntjoin(args, fasta=assemble.sources(args, fasta), w=w)
        nj.weights_list = set_weights(args)
        try:
            nj.load_minimizers_scaffold()
            nj.scaffold(keep=True)
            eng, tgt = nj._engine, len(nj._order) - 1
            pieces, first, ids = eng.scaffold_pieces()
            source_ids, source_len = eng.record_ids(tgt, eng.n_records(tgt)), eng.record_lengths(tgt)
        finally:
            nj.close()
    finally:
        os.chdir(cwd)
    rows, first = [tuple(int(x) for x in p) for p in pieces.tolist()], first.tolist()
    table = [rows[first[r]:first[r + 1]] for r in range(len(ids))]
    return dict(table=table, ids=ids, source_ids=source_ids, source_len=source_len, bed=make_bed(table, source_ids, source_len))


def make_bed(table, source_ids, source_len):
    seq = sorted((p for rec in table for p in rec if p[3] != R.GAP), key=lambda p: (p[0], p[1]))
    cut = [(p, q) for p, q in zip(seq, seq[1:]) if p[0] == q[0]]
    assert cut, "no contig of the misassembled target is cut"
    rev = [p for p in seq if p[3] == R.REV]
    assert rev, "no piece of the run is reverse-complemented"
    lines, n = [], 0

    def add(r, a, b, strand=b"+", name=None):
        nonlocal n
        lines.append(b"%s\t%d\t%d\t%s\t%d\t%s\n" % (name or source_ids[r].encode(), a, b, b"f%d" % n, n, strand))
        n += 1
    lines.append(b"track name=features\n")
    for p, q in cut:
        add(p[0], max(0, p[2] - 40), p[2] - 5)                        # left of the cut
        add(q[0], q[1] + 5, q[1] + 40, b"-")                  # right of it
        add(p[0], max(0, p[2] - 30), q[1] + 30)                       # across it, and across whatever was trimmed between the two pieces
        add(p[0], p[2] - 1, p[2])                             # the last base in front of it
    for p in rev[:2]:
        add(p[0], p[1] + 3, p[1] + 50)
        add(p[0], p[1] + 3, p[1] + 50, b"-")
        add(p[0], p[1], p[2], b".")                           # the whole piece
    for r, L in enumerate(source_len):
        add(r, 0, L)                                          # every contig whole
        add(r, 0, L + 1)                                      # ... and past its end
    add(0, 10, 20, name=b"no_such_contig")
    lines.append(source_ids[0].encode() + b"\t7\t9")          # three columns, no final newline
    return b"".join(lines)


def check_files(d, run, prefix="run", scaffolds=None, table=None, ids=None):
    "both files against the restatement; every lifted line against the bytes of the scaffolds and of the target"
    table, ids = table or run["table"], ids or run["ids"]
    src = [s.encode() for s in run["source_ids"]]
    want = R.lift_bed(table, run["source_len"], src, [i.encode() for i in ids], run["bed"])
    lifted, unlifted = (d / f"{prefix}.feat.lifted.bed").read_bytes(), (d / f"{prefix}.feat.unlifted.bed").read_bytes()
    assert (lifted, unlifted) == want[:2]
    st = want[2]
    assert st["whole"] and st["invalid"] and st["unknown"] == 1 and (st["split"] or st["partial"])
    contigs = read_fasta(os.path.join(FASTA, TARGET))
    scaffolds = scaffolds or dict(read_fasta(d / f"{OUT}.assigned.scaffolds.fa"), **read_fasta(d / f"{OUT}.unassigned.scaffolds.fa"))
    # the restatement's parts, in the order of the lifted lines
    features = [ln.split(b"\t") for ln in R.bed_lines(run["bed"]) if not ln.startswith(b"track")]
    parts = []
    for f in features:
        if f[0] in src and int(f[1]) < int(f[2]):
            for part in R.lift_one(table, run["source_len"], (src.index(f[0]), int(f[1]), int(f[2])))[1]:
                parts.append((f, part))
    lines = lifted.splitlines()
    assert len(lines) == len(parts) and len(lines) >= 10
    n_rev = 0
    for line, (f, (Rr, s, e, lo, rev)) in zip(lines, parts):
        c = line.split(b"\t")
        assert c[0].decode() == ids[Rr] and (int(c[1]), int(c[2])) == (s, e)
        want_text = contigs[f[0].decode()][lo:lo + e - s]
        assert scaffolds[ids[Rr]][s:e] == (rc(want_text) if rev else want_text), line
        if len(f) >= 6:
            assert c[3:5] == f[3:5] and c[5] == ({b"+": b"-", b"-": b"+"}.get(f[5], f[5]) if rev else f[5]), line
        n_rev += rev
    assert n_rev >= 1
    return want


def test_command_line(run, tmp_path):
    d = fresh(tmp_path, "cli")
    (d / "feat.bed").write_bytes(run["bed"])
    res = child(d, [sys.executable, "-m", "ntjoin_amd.assemble"] + argv("--lift", "feat.bed"))
    assert "feat.bed" in res.stderr and "lifted whole" in res.stderr
    want = check_files(d, run)
    # nothing else changes, and --lift_whole_only keeps the unlifted file and drops the parts of what is not WHOLE
    off = fresh(tmp_path, "off")
    child(off, [sys.executable, "-m", "ntjoin_amd.assemble"] + argv())
    for name in sorted(os.listdir(off)):
        if not os.path.islink(off / name):
            assert (d / name).read_bytes() == (off / name).read_bytes(), name
    assert sorted(set(os.listdir(d)) - set(os.listdir(off))) == ["feat.bed", "run.feat.lifted.bed", "run.feat.unlifted.bed"]
    whole = fresh(tmp_path, "whole")
    (whole / "feat.bed").write_bytes(run["bed"])
    child(whole, [sys.executable, "-m", "ntjoin_amd.assemble"] + argv("--lift", "feat.bed", "--lift_whole_only"))
    src = [s.encode() for s in run["source_ids"]]
    want_whole = R.lift_bed(run["table"], run["source_len"], src, [i.encode() for i in run["ids"]], run["bed"], whole_only=True)
    assert ((whole / "run.feat.lifted.bed").read_bytes(), (whole / "run.feat.unlifted.bed").read_bytes()) == want_whole[:2]
    assert want_whole[1] == want[1] and len(want_whole[0]) < len(want[0])


def test_make_front_end(run, tmp_path):
    d = fresh(tmp_path, "make")
    (d / "feat.bed").write_bytes(run["bed"])
    child(d, ["make", "-f", os.path.join(REPO, "ntJoin-mx"), "scaffold", f"target={TARGET}", f"references={REF}", "reference_weights=2", f"k={K}",
              f"w={W}", "n=1", "prefix=run", "overlap=False", "lift=feat.bed"])
    check_files(d, run, scaffolds=read_fasta(d / f"{OUT}.all.scaffolds.fa"))


def test_two_rounds(run, tmp_path):
    "the features lie on the contigs of the first target; the coordinates are the last round's scaffolds'"
    d = fresh(tmp_path, "rounds")
    (d / "feat.bed").write_bytes(run["bed"])
    child(d, [sys.executable, "-m", "ntjoin_amd.assemble"] + argv("--lift", "feat.bed", "--rounds_w", "50"))
    assert not os.path.exists(d / "run.feat.lifted.bed")   # earlier rounds lift nothing
    last = f"{OUT}.all.scaffolds.fa.k{K}.w50.n1"
    scaffolds = dict(read_fasta(d / f"{last}.assigned.scaffolds.fa"), **read_fasta(d / f"{last}.unassigned.scaffolds.fa"))
    # the composed table, as <p>.rounds.agp spells it
    index = {name: r for r, name in enumerate(run["source_ids"])}
    ids, table = [], []
    for line in (d / "run.rounds.agp").read_text().splitlines():
        c = line.split("\t")
        if not ids or ids[-1] != c[0]:
            ids.append(c[0])
            table.append([])
        if c[4] == "N":
            table[-1].append((0, 0, int(c[5]), R.GAP))
        else:
            table[-1].append((index[c[5]], int(c[6]) - 1, int(c[7]), R.REV if c[8] == "-" else R.FWD))
    assert ids == list(scaffolds)
    check_files(d, run, prefix="run.round2", scaffolds=scaffolds, table=table, ids=ids)
