"""CPU test of the writers' file side (ntjoin_amd/csrc/out_file.h): a small host program compiled against the header alone puts
blocks of a known pattern through OutFile::put into a regular file, stdout, a FIFO and a symbolic link, and prints put_parts for a
table whose expected values are written out by hand.  The program is built twice, plainly and with AddressSanitizer +
UndefinedBehaviorSanitizer (the runtime linked statically into the program; nothing is preloaded), and every case runs on both."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.conftest import REPO

CSRC = os.path.join(REPO, "ntjoin_amd", "csrc")
MIB = 1 << 20

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "out_file.h"
// parts                           : lines `bytes threads` on stdin -> put_parts, one per line, on stdout
// put PATH THREADS COMPLETE AFTER : lines `off bytes seed` on stdin, one put each; then close(), `complete` as told, and (AFTER = 1)
//                                   a line "after\n" through stdio's stdout
int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "parts")) {
        unsigned long long bytes;
        unsigned threads;
        while (scanf("%llu %u", &bytes, &threads) == 2) printf("%u\n", mxg::put_parts(bytes, threads));
        return 0;
    }
    if (argc != 6 || strcmp(argv[1], "put")) return 2;
    const unsigned threads = (unsigned)atoi(argv[3]);
    int rc = 0;
    {
        mxg::OutFile of;
        if (!of.open(argv[2])) return 3;
        unsigned long long off, bytes, seed;
        while (scanf("%llu %llu %llu", &off, &bytes, &seed) == 3) {
            std::vector<char> buf(bytes);
            for (unsigned long long i = 0; i < bytes; ++i) buf[i] = (char)((seed + 7 * i + (i >> 10)) & 255);
            if (!of.put(buf.data(), bytes, off, threads)) rc = 4;
        }
        if (!of.close()) rc = 5;
        if (!of.close()) rc = 6;  // (a second close is a success and does nothing)
        of.complete = atoi(argv[4]) != 0;
    }
    if (atoi(argv[5])) {
        fputs("after\n", stdout);
        if (fflush(stdout) != 0) rc = 7;
    }
    return rc;
}
"""


def pattern(n, seed):
    i = np.arange(n, dtype=np.uint64)
    return ((np.uint64(seed) + np.uint64(7) * i + (i >> np.uint64(10))) & np.uint64(255)).astype(np.uint8).tobytes()


def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    return cxx


def _sanitizer_flags(cxx, td):
    """-fsanitize with the runtime inside the program (so that its place among the loaded libraries does not matter), or None when
    the compiler cannot build and run such a program here"""
    probe = td / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"]):
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] + static
        exe = td / "probe"
        if subprocess.run([cxx] + flags + [str(probe), "-o", str(exe)], capture_output=True).returncode == 0 and \
                subprocess.run([str(exe)], capture_output=True).returncode == 0:
            return flags
    return None


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    td = tmp_path_factory.mktemp("out_file_" + request.param)
    cxx = _cxx()
    extra = []
    if request.param == "sanitized":
        extra = _sanitizer_flags(cxx, td)
        if extra is None:
            pytest.skip("the host compiler has no AddressSanitizer runtime to link")
    src, out = td / "out_file_prog.cpp", td / "out_file_prog"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread"] + extra + ["-I", CSRC, str(src), "-o", str(out)])
    return str(out)


def run_puts(exe, path, puts, threads=16, complete=1, after=0, **kw):
    lines = "".join("%d %d %d\n" % p for p in puts)
    return subprocess.run([exe, "put", path, str(threads), str(complete), str(after)], input=lines.encode(), capture_output=True,
                          timeout=60, **kw)


# bytes, threads -> parts = min(min(16, max(1, threads)), ceil(bytes / 1 MiB)), by hand
PARTS = [(0, 16, 0), (0, 0, 0), (0, 64, 0), (1, 16, 1), (MIB, 16, 1), (MIB + 1, 16, 2), (40 * MIB, 16, 16), (40 * MIB, 0, 1),
         (40 * MIB, 64, 16)]


def test_put_parts_on_a_table(exe):
    r = subprocess.run([exe, "parts"], input="".join("%d %d\n" % (b, t) for b, t, _ in PARTS), capture_output=True, text=True, check=True)
    assert [int(x) for x in r.stdout.split()] == [want for _, _, want in PARTS]


SIZES = [0, 1, MIB - 1, MIB, MIB + 1, 3 * MIB + 5]


def _layout(sizes):
    """(off, bytes, seed) of blocks laid side by side, and the file's image"""
    puts, image, off = [], b"", 0
    for s, n in enumerate(sizes):
        puts.append((off, n, 11 + 37 * s))
        image += pattern(n, 11 + 37 * s)
        off += n
    return puts, image


@pytest.mark.parametrize("threads", [1, 3, 16, 64])
def test_regular_file_out_of_order(exe, tmp_path, threads):
    puts, image = _layout(SIZES)
    path = tmp_path / "out.bin"
    order = [5, 0, 3, 1, 4, 2]  # (the last block first: the file grows beyond what has been written)
    r = run_puts(exe, str(path), [puts[i] for i in order], threads=threads)
    assert r.returncode == 0, r.stderr
    assert path.read_bytes() == image


GARBAGE = [1 << 40, 0, 12345, 7, (1 << 63) + 1, 3]  # offsets that mean nothing to a pipe


def test_stdout_takes_the_blocks_in_call_order(exe, tmp_path):
    puts, image = _layout(SIZES)
    (tmp_path / "-").write_bytes(b"a file called -")  # "-" is stdout, not this file: neither truncated nor removed
    r = run_puts(exe, "-", [(g, n, s) for g, (_, n, s) in zip(GARBAGE, puts)], complete=0, after=1, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert r.stdout == image + b"after\n"  # (stdout is still stdio's and still open after close())
    assert (tmp_path / "-").read_bytes() == b"a file called -"


def _read_fifo(fd):
    got = b""
    while True:
        part = os.read(fd, 1 << 16)  # (no writer left: an empty read is the end of file)
        if not part:
            return got
        got += part


@pytest.mark.parametrize("complete", [0, 1])
def test_fifo_takes_the_blocks_in_call_order_and_stays(exe, tmp_path, complete):
    puts, image = _layout([1, 0, 5000, 1, 30000])  # (under the pipe's 64 KiB: the writer never waits for this reader)
    fifo = tmp_path / "out.fifo"
    os.mkfifo(fifo)
    fd = os.open(fifo, os.O_RDONLY | os.O_NONBLOCK)
    try:
        r = run_puts(exe, str(fifo), [(g, n, s) for g, (_, n, s) in zip(GARBAGE, puts)], complete=complete)
        assert r.returncode == 0, r.stderr
        assert _read_fifo(fd) == image
    finally:
        os.close(fd)
    assert os.path.exists(fifo)


def test_incomplete_regular_file_is_removed_and_a_complete_one_stays(exe, tmp_path):
    puts, image = _layout([1, 5000])
    gone, stays = tmp_path / "gone.bin", tmp_path / "stays.bin"
    assert run_puts(exe, str(gone), puts, complete=0).returncode == 0
    assert run_puts(exe, str(stays), puts, complete=1).returncode == 0
    assert not gone.exists()
    assert stays.read_bytes() == image


def test_symbolic_link_to_a_regular_file_is_never_removed(exe, tmp_path):
    puts, image = _layout([1, 5000])
    target, link = tmp_path / "target.bin", tmp_path / "link.bin"
    target.write_bytes(b"old")
    os.symlink(target, link)
    assert run_puts(exe, str(link), puts, complete=0).returncode == 0
    assert link.is_symlink() and target.read_bytes() == image  # (written through the link at the blocks' offsets, and left alone)
