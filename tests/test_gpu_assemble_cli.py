"""GPU tests of the scaffolder's command line (`python -m ntjoin_amd.assemble`, `ntJoin-mx scaffold`): the files of the reference's
own run on its fixtures, the .path strings its tests pin, the AGP, the reference-TSV route and the make target.  Every run is a
child process under a time limit of its own; a test ends at the first one that does not return 0."""
import os
import subprocess
import sys

import pytest

from tests import _scaffold_cases as cases

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FASTA = os.path.join(cases.GOLDEN, "fasta")
EXPECTED = os.path.join(cases.GOLDEN, "scaffolds", "expected_f-f")
ENV = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
LIMIT = ["timeout", "-k", "10", "120"]
F_F = ["f-f_test.path", "f-f_test.scaf.f-f.fa.k32.w1000.tsv.unassigned.bed", "scaf.f-f.fa.k32.w1000.n1.assigned.scaffolds.fa",
       "scaf.f-f.fa.k32.w1000.n1.unassigned.scaffolds.fa"]

# the .path strings pinned in tests/test_gpu_adjust.py (the reference's tests/ntjoin_test.py, window 500, overlap off)
END_TO_END = [
    ("regions-ff-rr", "scaf.misassembled.f-f.r-r.fa", 1, False,
     ["2_1n-1_2p-:0-2232 20N 1_1p-2_2n-:2110-4489", "1_1p-2_2n+:0-1568 477N 2_1n-1_2p+:2712-4379"]),
    ("regions-ff-rr-nocut", "scaf.misassembled.f-f.r-r.fa", 1, True, ["2_1n-1_2p-:0-4379 20N 1_1p-2_2n-:0-4489"]),
    ("regions-fr-rf", "scaf.misassembled.f-r.r-f.fa", 2, False,
     ["2_1n-1_2n-:0-2232 253N 1_1p-2_2p+:2058-4489", "1_1p-2_2p+:0-1624 191N 2_1n-1_2n-:2518-4379"]),
    ("gap-dist", "scaf.multiple.fa", 1, False, ["2_1_p+:0-2492 100N 2_2_n-:0-2574", "1_1_p+:0-1744 124N 1_2_p+:0-1844"]),
]


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


def child(cwd, words):
    res = subprocess.run(LIMIT + words, cwd=cwd, env=ENV, capture_output=True, text=True, check=False)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    return res


def assemble(cwd, *argv):
    return child(cwd, [sys.executable, "-m", "ntjoin_amd.assemble"] + list(argv))


def link(tmp_path, *names):
    for name in names:
        os.symlink(os.path.join(FASTA, name), tmp_path / name)


def test_f_f_fixture_gives_the_reference_s_files(tmp_path):
    link(tmp_path, "scaf.f-f.fa", "ref.fa")
    assemble(tmp_path, "-p", "f-f_test", "-n", "1", "-s", "scaf.f-f.fa.k32.w1000.tsv", "-l", "1", "-r", "2", "-k", "32", "-t", "3", "--btllib_t", "2",
             "ref.fa.k32.w1000.tsv")
    for name in F_F:
        assert read(tmp_path / name) == read(os.path.join(EXPECTED, name)), name
    assert not os.path.exists(tmp_path / "f-f_test.agp")
    # the graph is the one ntjoin_amd.run writes from the sketches this run left behind
    child(tmp_path, [sys.executable, "-m", "ntjoin_amd.run", "-p", "run", "-n", "1", "-s", "scaf.f-f.fa.k32.w1000.tsv", "-l", "1", "-r", "2", "-k", "32",
                     "ref.fa.k32.w1000.tsv"])
    assert read(tmp_path / "f-f_test.mx.dot") == read(tmp_path / "run.mx.dot") and len(read(tmp_path / "run.mx.dot")) > 100


@pytest.mark.parametrize("name,target,n,no_cut,expected", END_TO_END, ids=[c[0] for c in END_TO_END])
def test_pinned_path_strings(name, target, n, no_cut, expected, tmp_path):
    link(tmp_path, target, "ref.multiple.fa")
    assemble(tmp_path, "-p", name + "_test", "-n", str(n), "-s", target + ".k32.w500.tsv", "-l", "1", "-r", "2", "-k", "32", "-g", "20", "-G", "0", "-m", "90",
             *(["--no_cut"] if no_cut else []), "ref.multiple.fa.k32.w500.tsv")
    lines = read(tmp_path / (name + "_test.path")).decode("ascii").splitlines()
    assert lines[0] == target
    got = [line.split("\t") for line in lines[1:]]
    # (which scaffold is ntJoin0 is not pinned: tests/test_gpu_adjust.py)
    assert [g[0] for g in got] == [f"ntJoin{i}" for i in range(len(expected))]
    assert sorted(g[1] for g in got) == sorted(expected)


def test_agp_flag_writes_the_pinned_lines(tmp_path):
    link(tmp_path, "scaf.f-f.termN.unassigned.fa", "ref.fa")
    assemble(tmp_path, "-p", "out", "-n", "1", "-s", "scaf.f-f.termN.unassigned.fa.k32.w1000.tsv", "-r", "2", "-k", "32", "--agp", "ref.fa.k32.w1000.tsv")
    assert read(tmp_path / "out.agp").decode("ascii").splitlines() == [
        "ntJoin0\t1\t1981\t1\tW\t1_f\t5\t1985\t+", "ntJoin0\t1982\t2001\t2\tN\t20\tscaffold\tyes\talign_genus",
        "ntJoin0\t2002\t4330\t3\tW\t2_f\t1\t2329\t+", "unassigned:0-14\t1\t8\t1\tW\tunassigned\t3\t10\t+"]


def test_an_existing_reference_tsv_is_loaded_not_sketched_again(tmp_path):
    link(tmp_path, "scaf.f-f.fa", "ref.fa")
    argv = ["-n", "1", "-s", "scaf.f-f.fa.k32.w1000.tsv", "-r", "2", "-k", "32", "ref.fa.k32.w1000.tsv"]
    assemble(tmp_path, "-p", "first", *argv)
    tsv = tmp_path / "ref.fa.k32.w1000.tsv"
    os.utime(tsv, ns=(10 ** 18, 10 ** 18))
    before = os.stat(tsv).st_mtime_ns
    first = {name: read(tmp_path / name.replace("f-f_test", "first")) for name in F_F}
    for name in F_F[2:]:
        os.remove(tmp_path / name)
    os.remove(tmp_path / "ref.fa")  # (only the sketch is left of the reference)
    assemble(tmp_path, "-p", "second", *argv)
    assert os.stat(tsv).st_mtime_ns == before
    assert {name: read(tmp_path / name.replace("f-f_test", "second")) for name in F_F} == first
    assert read(tmp_path / "second.mx.dot") == read(tmp_path / "first.mx.dot")


def test_make_scaffold_writes_the_files_and_their_concatenation(tmp_path):
    link(tmp_path, "scaf.f-f.fa", "ref.fa")
    child(tmp_path, ["make", "-f", os.path.join(REPO, "ntJoin-mx"), "scaffold", "target=scaf.f-f.fa", "references=ref.fa", "reference_weights=2", "k=32",
                     "w=1000", "n=1", "prefix=f-f_test", "overlap=False"])
    for name in F_F:
        assert read(tmp_path / name) == read(os.path.join(EXPECTED, name)), name
    assert read(tmp_path / "scaf.f-f.fa.k32.w1000.n1.all.scaffolds.fa") == read(os.path.join(EXPECTED, F_F[2])) + read(os.path.join(EXPECTED, F_F[3]))
    assert os.path.getsize(tmp_path / "f-f_test.mx.dot") > 100
