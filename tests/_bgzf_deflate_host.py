"""The stand-alone CPU program of the BGZF writer's tests: ntjoin_amd/csrc/bgzf_deflate.h (the member coder the kernel compiles too)
and bgzf_inflate.h built into one small host program with its own main, as tests/test_bgzf_cpu.py builds the decoder's.

    bgzf_deflate_host deflate <P> <text file> <bgzf file>

cuts the text into members of P bytes, codes each from an exact-size heap copy into an exact-size heap block (text + 31 bytes, 28
for the end marker: one byte outside either stops a sanitizer build), writes the chain with the end marker behind it, then reads
its own file back through bgzf_plan + bgzf_inflate_member and compares.  It prints `members M stored S bytes_in N bytes_out B`.
Exit status 0, or 3 + what went wrong."""
import os
import shutil
import subprocess

from tests.conftest import REPO

CSRC = os.path.join(REPO, "ntjoin_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "bgzf_deflate.h"
using namespace mxg;

struct Sink {
    uint8_t *p;
    uint32_t n = 0;
    void put(uint8_t b) { p[n++] = b; }
    uint8_t back(uint32_t d) const { return p[n - d]; }
};
static std::vector<unsigned char> slurp(const char *path)
{
    std::vector<unsigned char> v;
    FILE *fh = fopen(path, "rb");
    if (!fh) exit(2);
    unsigned char buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, fh)) > 0) v.insert(v.end(), buf, buf + got);
    fclose(fh);
    return v;
}
int main(int argc, char **argv)
{
    if (argc < 5 || strcmp(argv[1], "deflate")) return 1;
    const uint32_t P = (uint32_t)atoi(argv[2]);
    if (P < 1 || P > BGZF_MAX_PAYLOAD) return 1;
    const std::vector<unsigned char> text = slurp(argv[3]);
    std::vector<unsigned char> file;
    uint64_t members = 0, stored = 0;
    for (size_t lo = 0; lo < text.size(); lo += P) {
        const uint32_t n = (uint32_t)std::min<size_t>(P, text.size() - lo);
        std::unique_ptr<unsigned char[]> in(new unsigned char[n]);
        memcpy(in.get(), text.data() + lo, n);
        std::unique_ptr<unsigned char[]> out(new unsigned char[n + BGZF_SLACK]);
        bool st = false;
        const uint32_t size = bgzf_deflate_member_host(in.get(), n, out.get(), &st);
        if (size > n + BGZF_SLACK) return 4;
        file.insert(file.end(), out.get(), out.get() + size);
        ++members;
        stored += st ? 1 : 0;
    }
    {
        std::unique_ptr<unsigned char[]> out(new unsigned char[BGZF_EOF_BYTES]);
        if (bgzf_deflate_member_host(nullptr, 0, out.get()) != BGZF_EOF_BYTES) return 5;
        file.insert(file.end(), out.get(), out.get() + BGZF_EOF_BYTES);
    }
    FILE *fh = fopen(argv[4], "wb");
    if (!fh || fwrite(file.data(), 1, file.size(), fh) != file.size() || fclose(fh)) return 2;
    // back through this repository's own reader
    std::unique_ptr<unsigned char[]> exact(new unsigned char[file.size()]);
    memcpy(exact.get(), file.data(), file.size());
    BgzfPlan plan;
    if (!bgzf_plan(exact.get(), file.size(), plan)) return 6;
    if (plan.usz != text.size() || plan.members.size() != members || plan.n_all != members + 1) return 7;
    for (const BgzfMember &m : plan.members) {
        std::unique_ptr<uint8_t[]> back(new uint8_t[m.isize]);
        std::unique_ptr<unsigned char[]> in(new unsigned char[m.in_len]);
        memcpy(in.get(), exact.get() + m.in_off, m.in_len);
        BgzfHostSrc src{in.get(), m.in_len};
        Sink sink{back.get()};
        BgzfHostTab tab;
        if (bgzf_inflate_member(src, sink, tab, m.isize) != BGZF_OK) return 8;
        if (memcmp(back.get(), text.data() + m.out_off, m.isize) != 0) return 9;
        uint32_t crc = 0xFFFFFFFFu;
        for (uint32_t i = 0; i < m.isize; ++i) crc = bgzf_crc32_entry((crc ^ back[i]) & 255u) ^ (crc >> 8);
        if ((crc ^ 0xFFFFFFFFu) != m.crc) return 10;
        // ... and the CRC of the pieces put together as the kernel does: 255 bytes a piece
        uint32_t sum = 0;
        for (uint32_t lo = 0; lo < m.isize; lo += 255u) {
            const uint32_t hi = std::min(m.isize, lo + 255u);
            uint32_t c = lo ? 0u : 0xFFFFFFFFu;
            for (uint32_t i = lo; i < hi; ++i) c = bgzf_crc32_entry((c ^ back[i]) & 255u) ^ (c >> 8);
            sum ^= bgzf_crc_shift(c, m.isize - hi);
        }
        if ((sum ^ 0xFFFFFFFFu) != m.crc) return 11;
    }
    printf("members %llu stored %llu bytes_in %llu bytes_out %llu\n", (unsigned long long)members, (unsigned long long)stored,
           (unsigned long long)text.size(), (unsigned long long)file.size());
    return 0;
}
"""


def compiler():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    return cxx


def build(d, flags):
    """the program compiled in directory d (a pathlib.Path) with the given flags; returns its path"""
    src, exe = d / "bgzf_deflate_host.cpp", d / "bgzf_deflate_host"
    src.write_text(PROGRAM)
    subprocess.check_call([compiler(), "-std=c++17", "-Wall", "-Werror", "-I", CSRC, *flags, str(src), "-o", str(exe)])
    return str(exe)


def deflate(exe, payload, text, tmp_path, name="t"):
    """text -> (the BGZF file's bytes, {members, stored, bytes_in, bytes_out}) at `payload` bytes of text per member"""
    src, dst = tmp_path / (name + ".txt"), tmp_path / (name + ".gz")
    src.write_bytes(text)
    r = subprocess.run([exe, "deflate", str(payload), str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (name, payload, r.returncode, r.stderr[-2000:])
    f = r.stdout.split()
    return dst.read_bytes(), {f[i]: int(f[i + 1]) for i in range(0, len(f), 2)}
