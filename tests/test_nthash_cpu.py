"""CPU test of the device hash helpers (ntjoin_amd/csrc/nthash_dev.h) over the whole range of k the library accepts: the header's
text, unchanged, compiled for the host beside the stand-in headers of tools/nthash_shim and run by tools/nthash_check.cpp with the
library's own tables (csrc/nthash_tab.h) against the oracle's direct formula (oracle/mx_oracle.c, linked in).  Built plainly and
with AddressSanitizer + UndefinedBehaviorSanitizer (the runtime linked into the program; nothing is preloaded): every packed buffer
ends exactly 1 KiB behind its last base, which is what include/ntjoin_mx.h promises about a borrowed buffer."""
import os
import re
import shutil
import subprocess

import pytest

from tests.conftest import REPO
from tests.test_fai_cpu import _sanitizer_flags

CSRC = os.path.join(REPO, "ntjoin_amd", "csrc")
SHIM = os.path.join(REPO, "tools", "nthash_shim")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    td = tmp_path_factory.mktemp("nthash_check_" + request.param)
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc")
    assert cxx and cc, "no C/C++ compiler"
    extra = []
    if request.param == "sanitized":
        extra = _sanitizer_flags(cxx, td)
        if extra is None:
            pytest.skip("the host compiler has no AddressSanitizer runtime to link")
    # a quote include resolves beside the including file first: the header's copy stands beside the stand-in mxg_internal.h
    inc = td / "inc"
    shutil.copytree(SHIM, inc)
    shutil.copy(os.path.join(CSRC, "nthash_dev.h"), inc / "nthash_dev.h")
    shutil.copy(os.path.join(CSRC, "nthash_tab.h"), inc / "nthash_tab.h")
    with open(inc / "nthash_dev.h", "rb") as a, open(os.path.join(CSRC, "nthash_dev.h"), "rb") as b:
        assert a.read() == b.read()
    san = [f for f in extra if not f.startswith("-static")]
    obj = td / "mx_oracle.o"
    subprocess.check_call([cc, "-std=c11", "-O1", "-D_GNU_SOURCE", "-Wall"] + san + ["-c", os.path.join(REPO, "oracle", "mx_oracle.c"), "-o", str(obj)])
    out = td / "nthash_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas"] + extra +
                          ["-I", str(inc), "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "oracle"),
                           os.path.join(REPO, "tools", "nthash_check.cpp"), str(obj), "-o", str(out)])
    return str(out)


def test_device_helpers_equal_the_direct_formula_for_every_k(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    counts = dict(re.findall(r"^(\w+) (\d+)$", r.stdout, re.M))
    assert r.stdout.rstrip().endswith("OK")
    assert int(counts["k_sweep"]) >= 1024 * 48 == 49152     # every k in 1..1024 x first-base offsets 0..47
    assert int(counts["rolling"]) == 7 * 2000               # k in {1, 31, 32, 33, 64, 1023, 1024}, 2000 steps each
    assert int(counts["rotations"]) == 200 * 1101           # srol_var(n), n = 0..1100, on 200 values
    assert r.stderr == ""


def test_the_library_builds_its_tables_from_the_checked_header():
    "host_io.cpp's make_hash_tab / make_init_tab are the header's functions, and no second copy of the constants is left there"
    with open(os.path.join(CSRC, "host_io.cpp"), encoding="utf-8") as fh:
        text = fh.read()
    assert '#include "nthash_tab.h"' in text
    assert re.search(r"void make_hash_tab\(uint32_t k, HashTab \*t\) \{ nttab::hash_tab\(k, t->e\); \}", text)
    assert re.search(r"void make_init_tab\(uint32_t k, std::vector<uint4> &out\)\s*\{[^}]*nttab::init_tab\(out\);\s*\}", text)
    assert "0x3c8bfbb395c60474" not in text
