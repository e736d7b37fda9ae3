"""GPU tests of --gz on the scaffolder's command line (`python -m ntjoin_amd.assemble --gz`, `ntJoin-mx scaffold gz=True`) on the f-f
fixture: the scaffold FASTA files come out as BGZF (deflated on the device, ntjoin_amd/csrc/bgzf_deflate.hip), each decompresses to
the reference's own file, the concatenation is one BGZF chain with one end marker at its end, and no uncompressed scaffold FASTA is
left behind.  Every run is a child process under a time limit of its own."""
import gzip
import os
import struct
import subprocess
import sys

import pytest

from tests import _bgzf, _scaffold_cases as cases

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FASTA = os.path.join(cases.GOLDEN, "fasta")
EXPECTED = os.path.join(cases.GOLDEN, "scaffolds", "expected_f-f")
ENV = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
LIMIT = ["timeout", "-k", "10", "120"]
OUT = "scaf.f-f.fa.k32.w1000.n1"
TEXT = ["f-f_test.path", "f-f_test.scaf.f-f.fa.k32.w1000.tsv.unassigned.bed"]


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


def child(cwd, words):
    res = subprocess.run(LIMIT + words, cwd=cwd, env=ENV, capture_output=True, text=True, check=False)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    return res


def markers(data):
    "offsets of the members without text (end markers) in a BGZF file, walked by BSIZE"
    out, at = [], 0
    while at < len(data):
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        if data[at:at + size] == _bgzf.EOF_MARKER:
            out.append(at)
        at += size
    assert at == len(data)
    return out


def check_compressed(tmp_path, kinds):
    want = {kind: read(os.path.join(EXPECTED, f"{OUT}.{kind}.scaffolds.fa")) for kind in ("assigned", "unassigned")}
    want["all"] = want["assigned"] + want["unassigned"]
    for kind in kinds:
        data = read(tmp_path / f"{OUT}.{kind}.scaffolds.fa.gz")
        assert gzip.decompress(data) == want[kind], kind
        assert markers(data) == [len(data) - 28], kind                       # one end marker, at the end
        assert not os.path.exists(tmp_path / f"{OUT}.{kind}.scaffolds.fa")   # no uncompressed file beside it
    for name in TEXT:
        assert read(tmp_path / name) == read(os.path.join(EXPECTED, name)), name


def link(tmp_path):
    for name in ("scaf.f-f.fa", "ref.fa"):
        os.symlink(os.path.join(FASTA, name), tmp_path / name)


def test_assemble_gz(tmp_path):
    link(tmp_path)
    child(tmp_path, [sys.executable, "-m", "ntjoin_amd.assemble", "--gz", "-p", "f-f_test", "-n", "1", "-s", "scaf.f-f.fa.k32.w1000.tsv", "-l", "1",
                     "-r", "2", "-k", "32", "ref.fa.k32.w1000.tsv"])
    check_compressed(tmp_path, ("assigned", "unassigned"))


def test_make_scaffold_gz(tmp_path):
    link(tmp_path)
    child(tmp_path, ["make", "-f", os.path.join(REPO, "ntJoin-mx"), "scaffold", "gz=True", "target=scaf.f-f.fa", "references=ref.fa",
                     "reference_weights=2", "k=32", "w=1000", "n=1", "prefix=f-f_test", "overlap=False"])
    check_compressed(tmp_path, ("assigned", "unassigned", "all"))
