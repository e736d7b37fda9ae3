"""--gz on the command line of ntjoin_amd.run / ntjoin_amd.assemble (the reference's parser has no such flag): a store-true flag
that is off by default, and the `gz` variable of `ntJoin-mx scaffold`, which adds it and makes the .fa.gz concatenation."""
import os
import subprocess

from ntjoin_amd.run import parse_arguments
from tests.conftest import REPO

ARGV = ["-s", "t.fa.k32.w100.tsv", "-r", "2", "-k", "32", "r.fa.k32.w100.tsv"]


def test_gz_is_a_store_true_flag_off_by_default():
    assert parse_arguments(ARGV).gz is False
    assert parse_arguments(["--gz"] + ARGV).gz is True
    assert parse_arguments(ARGV + ["--gz"]).gz is True


def dry(*words):
    return subprocess.run(["make", "-n", "-f", os.path.join(REPO, "ntJoin-mx"), "scaffold", "target=t.fa", "references=r.fa", "reference_weights=2",
                           "k=32", "w=100", *words], capture_output=True, text=True, check=True, timeout=60).stdout


def test_make_variable_adds_the_flag_and_the_compressed_concatenation():
    plain, comp = dry(), dry("gz=True")
    assert dry("gz=False") == plain and "--gz" not in plain and ".gz" not in plain
    assert " --gz " in comp
    assert "head -c -28 t.fa.k32.w100.n1.assigned.scaffolds.fa.gz && cat t.fa.k32.w100.n1.unassigned.scaffolds.fa.gz; } > t.fa.k32.w100.n1.all.scaffolds.fa.gz" in comp
    assert "all.scaffolds.fa\n" not in comp
