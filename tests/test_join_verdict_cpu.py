"""CPU test of the partitioned join's verdict words (ntjoin_amd/csrc/join_verdict.h): a small host program compiled against the
header prints its constants and evaluates its predicate on the words this test feeds it.  Expected values are worked out here, in
Python, from the rule the kernels had before the header existed: the verdict word is (item << 3) | flags with MXG_MX_UNIQUE = 1,
MXG_MX_SHARED = 2, MXG_MX_INALL = 4.
(The header holds no record hash: carrying the key's product in the records was measured and not shipped)"""
import os
import shutil
import subprocess

from tests.conftest import REPO

CSRC = os.path.join(REPO, "ntjoin_amd", "csrc")
INCLUDE = os.path.join(REPO, "include")
UNIQUE, SHARED, INALL = 1, 2, 4

PROGRAM = r"""
#include <cinttypes>
#include <cstdio>
#include "join_verdict.h"
using namespace mxg;
int main()
{
    printf("%u %u %u\n", PJ_VERDICT_PREFILL, PJ_VERDICT_REF, (unsigned)MXG_MX_UNIQUE);
    uint64_t v;
    while (scanf("%" SCNu64, &v) == 1) printf("%d\n", pj_verdict_is_prefill((uint32_t)v) ? 1 : 0);
    return 0;
}
"""

def _run(lines, tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    src, exe = tmp_path / "join_verdict.cpp", tmp_path / "join_verdict"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-I", INCLUDE, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    return [list(map(int, l.split())) for l in out.splitlines()]


def test_prefill_word_and_constants(tmp_path):
    head = _run([], tmp_path)[0]
    assert head[0] == UNIQUE == head[2]   # the prefill is MXG_MX_UNIQUE: once in its assembly, not in every assembly
    assert head[1] == SHARED              # a reference: SHARED without UNIQUE, which no verdict is


def test_predicate_is_true_for_the_prefill_alone(tmp_path):
    words = []
    for fl in range(8):              # all eight flag combinations, without and with an item index above them
        for item in (0, 1, 2, 5, 0x1FFFFFFF):
            words.append((item << 3) | fl)
    for item in (0, 1, 77, 0x1FFFFFFF):  # references (PJ_VERDICT_REF in the low bits)
        words.append((item << 3) | 2)
    words.append(0)                  # the word of a failed stage / a record beyond the capacity
    got = _run([str(w) for w in words], tmp_path)[1:]
    assert len(got) == len(words)
    for w, (g,) in zip(words, got):
        assert g == (1 if w == UNIQUE else 0), hex(w)
    assert sum(g for (g,) in got) == 1
