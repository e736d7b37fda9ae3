"""GPU tests of --fai on the scaffolder's command line (`python -m ntjoin_amd.assemble --fai`, `ntJoin-mx scaffold fai=True`) on the f-f
fixture: the inputs' indexes equal the reference's recorded `samtools faidx` outputs (tests/golden/fai/), the indexes of the scaffold
files and of their concatenation equal the restatement over those files, with gz=True the .gzi of the `all` file gives random access
across the seam between its two parts, and without the flag no index appears and nothing else changes.  Every run is a child process
under a time limit of its own."""
import gzip
import os
import subprocess
import sys

import pytest

from tests import _fai_restatement as R, _scaffold_cases as cases
from tests.test_gpu_fai import check_random_access, members_of, read

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FASTA = os.path.join(cases.GOLDEN, "fasta")
GOLDEN_FAI = os.path.join(cases.GOLDEN, "fai")
EXPECTED = os.path.join(cases.GOLDEN, "scaffolds", "expected_f-f")
ENV = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
LIMIT = ["timeout", "-k", "10", "120"]
OUT = "scaf.f-f.fa.k32.w1000.n1"
ASSEMBLE = [sys.executable, "-m", "ntjoin_amd.assemble", "-p", "f-f_test", "-n", "1", "-s", "scaf.f-f.fa.k32.w1000.tsv", "-l", "1", "-r", "2", "-k", "32",
            "ref.fa.k32.w1000.tsv"]
MAKE = ["make", "-f", os.path.join(REPO, "ntJoin-mx"), "scaffold", "target=scaf.f-f.fa", "references=ref.fa", "reference_weights=2", "k=32", "w=1000",
        "n=1", "prefix=f-f_test", "overlap=False"]


def child(cwd, words):
    res = subprocess.run(LIMIT + words, cwd=cwd, env=ENV, capture_output=True, text=True, check=False)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    return res


def fresh(tmp_path, name):
    d = tmp_path / name
    d.mkdir()
    for fa in ("scaf.f-f.fa", "ref.fa"):
        os.symlink(os.path.join(FASTA, fa), d / fa)
    return d


def files(d):
    return {n: read(d / n) for n in sorted(os.listdir(d)) if not os.path.islink(d / n)}


def check_inputs(d):
    for fa in ("scaf.f-f.fa", "ref.fa"):
        assert read(d / (fa + ".fai")) == read(os.path.join(GOLDEN_FAI, fa + ".fai")), fa
        assert not os.path.exists(d / (fa + ".gzi"))


def test_assemble_fai(tmp_path):
    off, on = fresh(tmp_path, "off"), fresh(tmp_path, "on")
    child(off, ASSEMBLE)
    child(on, ASSEMBLE + ["--fai"])
    before, after = files(off), files(on)
    assert not [n for n in before if n.endswith((".fai", ".gzi"))]
    assert {n: v for n, v in after.items() if not n.endswith(".fai")} == before  # every other file is unchanged
    check_inputs(on)
    for kind in ("assigned", "unassigned"):
        text = after[f"{OUT}.{kind}.scaffolds.fa"]
        assert text == read(os.path.join(EXPECTED, f"{OUT}.{kind}.scaffolds.fa"))
        assert after[f"{OUT}.{kind}.scaffolds.fa.fai"] == R.fai_bytes(text)
    assert sorted(n for n in after if n.endswith(".fai")) == sorted(
        ["ref.fa.fai", "scaf.f-f.fa.fai", f"{OUT}.assigned.scaffolds.fa.fai", f"{OUT}.unassigned.scaffolds.fa.fai"])


def test_a_reference_from_its_tsv_gets_a_line_on_stderr(tmp_path):
    d = fresh(tmp_path, "run")
    child(d, ASSEMBLE)  # (leaves ref.fa.k32.w1000.tsv: the next run loads it)
    res = child(d, ASSEMBLE + ["--fai"])
    assert "ref.fa.k32.w1000.tsv was loaded from its TSV: no FASTA index is written for it" in res.stderr
    assert not os.path.exists(d / "ref.fa.fai")
    assert read(d / "scaf.f-f.fa.fai") == read(os.path.join(GOLDEN_FAI, "scaf.f-f.fa.fai"))


def test_make_scaffold_fai(tmp_path):
    off, on = fresh(tmp_path, "off"), fresh(tmp_path, "on")
    child(off, MAKE)
    child(on, MAKE + ["fai=True"])
    before, after = files(off), files(on)
    assert not [n for n in before if n.endswith((".fai", ".gzi"))]
    assert {n: v for n, v in after.items() if not n.endswith(".fai")} == before
    check_inputs(on)
    for kind in ("assigned", "unassigned", "all"):
        assert after[f"{OUT}.{kind}.scaffolds.fa.fai"] == R.fai_bytes(after[f"{OUT}.{kind}.scaffolds.fa"]), kind


def test_make_scaffold_fai_gz(tmp_path):
    d = fresh(tmp_path, "run")
    child(d, MAKE + ["fai=True", "gz=True"])
    check_inputs(d)
    for kind in ("assigned", "unassigned", "all"):
        blob = read(d / f"{OUT}.{kind}.scaffolds.fa.gz")
        text = gzip.decompress(blob)
        assert read(d / f"{OUT}.{kind}.scaffolds.fa.gz.fai") == R.fai_bytes(text), kind
        gzi = read(d / f"{OUT}.{kind}.scaffolds.fa.gz.gzi")
        assert gzi == R.gzi_bytes(members_of(blob)), kind
        if text:  # (the f-f run leaves nothing unassigned)
            check_random_access(blob, gzi, text)
    # the seam: the unassigned part's first member has a pair of its own in the `all` file (when that part holds text; the seam
    # inside a file of many members: tests/test_gpu_fai.py::test_scaffold_indexes_with_borders_inside_records)
    first, second = (gzip.decompress(read(d / f"{OUT}.{kind}.scaffolds.fa.gz")) for kind in ("assigned", "unassigned"))
    assert (len(first) in [u for _, u in R.parse_gzi(read(d / f"{OUT}.all.scaffolds.fa.gz.gzi"))]) == bool(second)
