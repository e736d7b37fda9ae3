"""GPU tests of --synteny on the command line (`python -m ntjoin_amd.assemble`), on the reference's own fixtures under
tests/golden/fasta at k = 32 and w = 100: <prefix>.synteny.paf against the restatement of the contract
(tests/_synteny_restatement.py) applied to the graph arrays and the scaffolds' piece table read through the Python API; against the
written text alone -- the k-mer of the scaffold at either end of every line is the k-mer of the reference there, or its reverse
complement; coordinates inside the lengths the .fai files give; nothing else changes in a run; --gz and --rounds_w; a reference given
as TSV with and without its .fai.  Every run is a child process under a time limit of its own."""
import glob
import gzip
import os
import shutil
import subprocess
import sys

import pytest

from tests import _synteny_restatement as R
from tests.conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu

FASTA = os.path.join(GOLDEN, "fasta")
ENV = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
LIMIT = ["timeout", "-k", "10", "120"]
K, W = 32, 100
# (ref.fa shares no unique minimizer with the misassembled fixture, whose two records each spell both records of ref.multiple.fa: that
# run's graph is empty and its PAF has no line, so the fixture is also run against the reference it was made from)
RUNS = [("ref.fa", "scaf.f-f.fa"), ("ref.fa", "scaf.f-r.fa"), ("ref.fa", "scaf.r-r.fa"), ("ref.fa", "scaf.misassembled.f-r.r-f.fa"),
        ("ref.multiple.fa", "scaf.misassembled.f-r.r-f.fa")]
EMPTY = [("ref.fa", "scaf.misassembled.f-r.r-f.fa")]
SYN = ["--synteny", "--synteny_min_anchors", "2"]
COMP = str.maketrans("ACGT", "TGCA")


def argv(target, *opts, ref="ref.fa"):
    return ["-p", "run", "-n", "1", "-s", f"{target}.k{K}.w{W}.tsv", "-l", "1", "-r", "2", "-k", str(K)] + list(opts) + [f"{ref}.k{K}.w{W}.tsv"]


def child(cwd, words):
    res = subprocess.run(LIMIT + [sys.executable, "-m", "ntjoin_amd.assemble"] + words, cwd=cwd, env=ENV, capture_output=True, text=True, check=False)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    return res


def fresh(tmp_path, name, target, ref="ref.fa"):
    d = tmp_path / name
    d.mkdir()
    for fa in (target, ref):
        os.symlink(os.path.join(FASTA, fa), d / fa)
    return d


def files(d):
    return {n: open(d / n, "rb").read() for n in sorted(os.listdir(d)) if not os.path.islink(d / n)}


def read_fasta(path):
    opener = gzip.open if str(path).endswith(".gz") else open
    seqs, name = {}, None
    with opener(path, "rt") as fh:
        for line in fh:
            if line.startswith(">"):
                name = line[1:].split()[0]
                assert name not in seqs
                seqs[name] = []
            else:
                seqs[name].append(line.strip())
    return {n: "".join(parts) for n, parts in seqs.items()}


def paf_rows(text):
    rows = []
    for line in text.splitlines():
        c = line.split("\t")
        assert len(c) == 13 and c[11] == "255" and c[12].startswith("cm:i:") and c[4] in "+-"
        rows.append((c[0], int(c[1]), int(c[2]), int(c[3]), c[4], c[5], int(c[6]), int(c[7]), int(c[8]), int(c[9]), int(c[10]), int(c[12][5:])))
    return rows


def same_kmer(a, b):
    a, b = a.upper(), b.upper()
    return len(a) == K and (a == b or a == b.translate(COMP)[::-1])


def check_against_text(paf_text, scaffolds, ref, fai_lengths=None):
    "(b) and (c): every line against the written sequences alone"
    rows = paf_rows(paf_text)
    for qname, qlen, qs, qe, strand, tname, tlen, ts, te, matches, blocklen, n in rows:
        q, t = scaffolds[qname], ref[tname]
        assert 0 <= qs < qe <= qlen == len(q) and 0 <= ts < te <= tlen == len(t)
        if fai_lengths is not None:
            assert fai_lengths[qname] == qlen
        first, last = (t[ts:ts + K], t[te - K:te]) if strand == "+" else (t[te - K:te], t[ts:ts + K])
        assert same_kmer(q[qs:qs + K], first), (qname, qs, strand, tname, ts, te)
        assert same_kmer(q[qe - K:qe], last), (qname, qe, strand, tname, ts, te)
        assert n >= 2 and matches == min(n * K, qe - qs, te - ts) and blocklen == max(qe - qs, te - ts)
    return rows


def fai_lengths(*paths):
    out = {}
    for p in paths:
        for line in open(p, encoding="utf-8"):
            c = line.split("\t")
            out[c[0]] = int(c[1])
    return out


def restated_paf(d, target, opts, monkeypatch, ref="ref.fa"):
    "(a) the same run in-process without --synteny: the restatement over get_graph and scaffold_pieces, as PAF text"
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
        rows, first = pieces.tolist(), first.tolist()
        want = R.synteny(g["vertex_pos"], g["vertex_record"], 1, 0, K, max_gap=100000, min_anchors=2, min_span=0, pieces=rows, first=first)
        return R.paf(want["blocks"], ids, R.query_lengths(None, rows, first), eng.record_ids(0, eng.n_records(0)), eng.record_lengths(0), K)
    finally:
        nj.close()


@pytest.mark.parametrize("ref,target", RUNS, ids=[f"{r}-{t}" for r, t in RUNS])
@pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "plain"])
def test_paf_of_a_run(ref, target, overlap, tmp_path, monkeypatch):
    opts = ["--overlap"] if overlap else []
    on, off, inproc = fresh(tmp_path, "on", target, ref), fresh(tmp_path, "off", target, ref), fresh(tmp_path, "inproc", target, ref)
    child(on, argv(target, "--fai", *opts, *SYN, ref=ref))
    child(off, argv(target, "--fai", *opts, ref=ref))
    # (d) nothing else changes
    before, after = files(off), files(on)
    assert not any(n.endswith(".paf") for n in before)
    assert {n: v for n, v in after.items() if n != "run.synteny.paf"} == before and "run.synteny.paf" in after
    paf = after["run.synteny.paf"].decode("ascii")
    # (a) the restatement over the arrays the Python API hands out
    assert paf == restated_paf(inproc, target, opts, monkeypatch, ref)
    # (b), (c) the text of the scaffolds and of the reference
    out = f"{target}.k{K}.w{W}.n1"
    scaffolds = dict(read_fasta(on / f"{out}.assigned.scaffolds.fa"), **read_fasta(on / f"{out}.unassigned.scaffolds.fa"))
    lengths = fai_lengths(on / f"{out}.assigned.scaffolds.fa.fai", on / f"{out}.unassigned.scaffolds.fa.fai")
    rows = check_against_text(paf, scaffolds, read_fasta(os.path.join(FASTA, ref)), lengths)
    assert bool(rows) == ((ref, target) not in EMPTY)
    if target == "scaf.f-f.fa":
        assert any(r[0].startswith("ntJoin") for r in rows)
    if ref == "ref.multiple.fa":
        assert {r[5] for r in rows} == set(read_fasta(os.path.join(FASTA, ref)))   # both records of the reference are reached


def test_defaults_gz_and_rounds(tmp_path):
    "(e) --gz and --rounds_w leave a PAF that fits the files of that run; the defaults of the three parameters"
    target = "scaf.f-r.fa"
    ref = read_fasta(os.path.join(FASTA, "ref.fa"))
    out = f"{target}.k{K}.w{W}.n1"
    gz = fresh(tmp_path, "gz", target)
    child(gz, argv(target, "--overlap", "--gz", *SYN))
    scaffolds = dict(read_fasta(gz / f"{out}.assigned.scaffolds.fa.gz"), **read_fasta(gz / f"{out}.unassigned.scaffolds.fa.gz"))
    assert check_against_text((gz / "run.synteny.paf").read_text(), scaffolds, ref)
    plain = fresh(tmp_path, "plain", target)
    child(plain, argv(target, "--overlap", *SYN))
    assert (plain / "run.synteny.paf").read_bytes() == (gz / "run.synteny.paf").read_bytes()
    dflt = fresh(tmp_path, "dflt", target)
    child(dflt, argv(target, "--overlap", "--synteny"))
    kept = [r for r in paf_rows((plain / "run.synteny.paf").read_text()) if r[11] >= 3]
    assert paf_rows((dflt / "run.synteny.paf").read_text()) == kept
    rounds = fresh(tmp_path, "rounds", target)
    child(rounds, argv(target, "--overlap", "--rounds_w", "50", *SYN))
    assert sorted(glob.glob(str(rounds / "*.paf"))) == [str(rounds / "run.round2.synteny.paf")]
    last = f"{out}.all.scaffolds.fa.k{K}.w50.n1"
    scaffolds = dict(read_fasta(rounds / f"{last}.assigned.scaffolds.fa"), **read_fasta(rounds / f"{last}.unassigned.scaffolds.fa"))
    assert check_against_text((rounds / "run.round2.synteny.paf").read_text(), scaffolds, ref)


def test_reference_given_as_tsv(tmp_path):
    "(f) no lengths in the handle: skipped with one line on stderr without <fasta>.fai, used with it"
    target = "scaf.f-f.fa"
    d = fresh(tmp_path, "d", target)
    first = child(d, argv(target, "--fai", *SYN))   # sketches the reference, leaves its TSV and its .fai
    assert "synteny PAF" not in first.stderr and os.path.exists(d / f"ref.fa.k{K}.w{W}.tsv")
    want = (d / "run.synteny.paf").read_bytes()
    assert want
    shutil.move(d / "ref.fa.fai", d / "kept.fai")
    second = child(d, argv(target, *SYN))
    assert f"ntjoin_amd: ref.fa.k{K}.w{W}.tsv was loaded from its TSV and its FASTA has no .fai: the synteny PAF has no lines for it" in second.stderr
    assert (d / "run.synteny.paf").read_bytes() == b""
    shutil.move(d / "kept.fai", d / "ref.fa.fai")
    third = child(d, argv(target, *SYN))
    assert "synteny PAF" not in third.stderr and (d / "run.synteny.paf").read_bytes() == want
