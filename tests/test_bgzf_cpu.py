"""CPU tests of the BGZF decoder the device route compiles into its kernel (ntjoin_amd/csrc/bgzf_inflate.h): the member walk and the
raw DEFLATE decoder, built into a small host program as tests/test_sel_requests_cpu.py builds its header.

 - the helper's files (tests/_bgzf.py) are what Python's gzip reads back, and the levels / strategies used really reach the stored,
   the fixed-Huffman and the dynamic-Huffman decoder (first block type 00, 01, 10);
 - the program inflates every decoder shape and member size of the GPU tests and gives the text zlib compressed;
 - a few thousand seeded corruptions of small members (bit flips, cut files, cut members, wrong ISIZE, deflate data replaced by
   random bytes): each ends refused by the walk, with a decoder status, with a CRC that does not match, or -- a flip in a byte that
   carries no meaning, the header's time stamp or the padding bits behind the last code -- with the original text (a cut that falls
   exactly between two members: with the text up to there, a BGZF file in its own right); never
   with another text, a crash or an endless loop.  The program counts the decoder's steps itself and checks them against the bound
   bgzf_inflate.h states (8 x deflate bytes + 1);
 - the same program built with -fsanitize=address,undefined (its own main, no preload) repeats both: source and sink are heap
   blocks of exactly the member's sizes, so one byte read or written outside them stops it."""
import gzip
import os
import shutil
import subprocess
import zlib

import pytest

from tests import _bgzf
from tests.conftest import REPO

CSRC = os.path.join(REPO, "ntjoin_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "bgzf_inflate.h"
using namespace mxg;

struct Sink {  // writes without a check of its own: the decoder's are under test (the block has exactly ISIZE bytes)
    uint8_t *p;
    uint32_t n = 0, crc = 0xFFFFFFFFu;
    const uint32_t *tab;
    void put(uint8_t b)
    {
        p[n++] = b;
        crc = tab[(crc ^ b) & 255u] ^ (crc >> 8);
    }
    uint8_t back(uint32_t d) const { return p[n - d]; }
};
static uint32_t crc_tab[256];
static uint64_t budget_broken = 0, max_steps = 0;

// one member from exact-size heap copies; status as the kernel forms it (decoder status, then the CRC)
static uint32_t inflate_one(const unsigned char *file, const BgzfMember &m, std::string *text)
{
    std::unique_ptr<unsigned char[]> in(new unsigned char[m.in_len ? m.in_len : 1]);
    memcpy(in.get(), file + m.in_off, m.in_len);
    std::unique_ptr<uint8_t[]> out(new uint8_t[m.isize ? m.isize : 1]);
    BgzfHostSrc src{in.get(), m.in_len};
    Sink sink{out.get(), 0, 0xFFFFFFFFu, crc_tab};
    BgzfHostTab tab;
    uint32_t steps = 0;
    uint32_t st = bgzf_inflate_member(src, sink, tab, m.isize, &steps);
    if ((uint64_t)steps > 8ull * m.in_len + 1ull) ++budget_broken;
    if (steps > max_steps) max_steps = steps;
    if (st == BGZF_OK && (sink.crc ^ 0xFFFFFFFFu) != m.crc) st = BGZF_CRC;
    if (st == BGZF_OK && text) text->append(reinterpret_cast<const char *>(out.get()), m.isize);
    return st;
}
// 0: refused by the walk, 1: a member's status, 2: a member's CRC, 3: inflated (text filled)
static int inflate_file(const std::vector<unsigned char> &f, std::string &text, uint32_t *status)
{
    std::unique_ptr<unsigned char[]> exact(new unsigned char[f.size() ? f.size() : 1]);
    memcpy(exact.get(), f.data(), f.size());
    BgzfPlan plan;
    text.clear();
    *status = 0;
    if (!bgzf_plan(exact.get(), f.size(), plan)) return 0;
    for (const BgzfMember &m : plan.members) {
        if (m.in_off + m.in_len > f.size() || m.out_off != text.size()) abort();
        if ((*status = inflate_one(exact.get(), m, &text)) != BGZF_OK) return *status == BGZF_CRC ? 2 : 1;
    }
    if (text.size() != plan.usz) abort();
    return 3;
}
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
static uint64_t rng_state;
static uint32_t rnd(uint32_t n)  // xorshift64*, [0, n)
{
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)(((rng_state * 2685821657736338717ull) >> 33) % n);
}
int main(int argc, char **argv)
{
    for (uint32_t i = 0; i < 256; ++i) crc_tab[i] = bgzf_crc32_entry(i);
    if (argc >= 3 && !strcmp(argv[1], "inflate")) {  // the text to stdout; exit status 10 + outcome unless inflated
        std::string text;
        uint32_t status;
        const int r = inflate_file(slurp(argv[2]), text, &status);
        if (r != 3) {
            fprintf(stderr, "outcome %d status %u\n", r, status);
            return 10 + r;
        }
        fwrite(text.data(), 1, text.size(), stdout);
        fprintf(stderr, "steps_max %llu budget_broken %llu\n", (unsigned long long)max_steps, (unsigned long long)budget_broken);
        return budget_broken ? 9 : 0;
    }
    if (argc >= 5 && !strcmp(argv[1], "fuzz")) {  // file seed trials
        const std::vector<unsigned char> good = slurp(argv[2]);
        rng_state = strtoull(argv[3], nullptr, 10) * 2 + 1;
        const uint32_t trials = (uint32_t)atoi(argv[4]);
        std::string want, text;
        uint32_t status;
        if (inflate_file(good, want, &status) != 3 || good.size() < 64) return 3;
        BgzfPlan plan;
        bgzf_plan(good.data(), good.size(), plan);
        uint64_t outcome[4] = {0, 0, 0, 0}, same = 0, prefix = 0, other = 0, by_status[16] = {};
        for (uint32_t t = 0; t < trials; ++t) {
            std::vector<unsigned char> f = good;
            const BgzfMember &m = plan.members[rnd((uint32_t)plan.members.size())];
            const uint64_t trailer = m.in_off + m.in_len;
            const uint32_t kind = rnd(6);
            if (kind == 0) {  // one bit anywhere in the file
                f[rnd((uint32_t)f.size())] ^= (unsigned char)(1u << rnd(8));
            } else if (kind == 1) {  // one byte of a member's deflate data
                f[m.in_off + rnd(m.in_len)] ^= (unsigned char)(1u + rnd(255));
            } else if (kind == 2) {  // the file cut short
                f.resize(rnd((uint32_t)f.size()));
            } else if (kind == 3) {  // ISIZE: another value of at most 65536 (the walk lets it pass)
                uint32_t v = rnd(2) ? m.isize + 1 + rnd(3) : rnd(m.isize);
                if (v > 65536) v = m.isize - 1;
                for (int b = 0; b < 4; ++b) f[trailer + 4 + b] = (unsigned char)(v >> (8 * b));
            } else if (kind == 4) {  // the deflate data of a member: random bytes from some place on
                for (uint64_t i = m.in_off + rnd(m.in_len); i < trailer; ++i) f[i] = (unsigned char)rnd(256);
            } else {  // the deflate data ends early: the member's last bytes become its trailer (the walk's sizes stay right)
                const uint32_t cut = 1 + rnd(m.in_len < 9 ? m.in_len : 8);
                std::vector<unsigned char> g(f.begin(), f.begin() + (long)(trailer - cut));
                g.insert(g.end(), f.begin() + (long)trailer, f.end());
                // BSIZE of this member: 16 bits at its header's offset 16 (the member starts in_off - 18 bytes)
                const uint64_t h0 = m.in_off - 18;
                const uint32_t bs = ((uint32_t)g[h0 + 16] | (uint32_t)g[h0 + 17] << 8) - cut;
                g[h0 + 16] = (unsigned char)bs;
                g[h0 + 17] = (unsigned char)(bs >> 8);
                f.swap(g);
            }
            const int r = inflate_file(f, text, &status);
            ++outcome[r];
            if (r == 1 || r == 2) ++by_status[status & 15u];
            // (a file cut at a member's border is a BGZF file of fewer members: zlib reads it as that too)
            const bool cut_at_border = kind == 2 && text.size() < want.size() && want.compare(0, text.size(), text) == 0;
            if (r == 3) ++(text == want ? same : cut_at_border ? prefix : other);
        }
        printf("trials %u refused %llu status %llu crc %llu same %llu prefix %llu other %llu budget_broken %llu steps_max %llu\n", trials,
               (unsigned long long)outcome[0], (unsigned long long)outcome[1], (unsigned long long)outcome[2], (unsigned long long)same,
               (unsigned long long)prefix, (unsigned long long)other, (unsigned long long)budget_broken, (unsigned long long)max_steps);
        printf("by_status");
        for (int s = 1; s < 12; ++s) printf(" %llu", (unsigned long long)by_status[s]);
        printf("\n");
        return 0;
    }
    return 1;
}
"""


def _compiler():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    return cxx


def _build(d, flags):
    src, exe = d / "bgzf_host.cpp", d / "bgzf_host"
    src.write_text(PROGRAM)
    subprocess.check_call([_compiler(), "-std=c++17", "-Wall", "-Werror", "-I", CSRC, *flags, str(src), "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("bgzf_host"), ["-O2"])


@pytest.fixture(scope="module")
def program_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("bgzf_host_san"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


@pytest.fixture(scope="module")
def texts():
    return {"shapes": _bgzf.shapes_fasta(), "decoder": _bgzf.decoder_fasta()}


# (name, text, write_bgzf arguments): every member size of the text-shape tests and every decoder shape of the GPU tests
def _cases(texts):
    shapes, dec = texts["shapes"], texts["decoder"]
    rnd = [_bgzf.RND_AT, _bgzf.RND_LEN] + [60000] * 40
    cases = [("size1", shapes[:30000], dict(payload_sizes=1)),
             ("size100", shapes, dict(payload_sizes=100)),
             ("size4096", shapes, dict(payload_sizes=4096)),
             ("size65280", shapes, dict(payload_sizes=65280)),
             ("cycle", shapes, dict(payload_sizes=(0, 1, 65280, 7, 0, 30000))),
             ("no_eof", shapes, dict(payload_sizes=4096, eof=False)),
             ("one_byte", b">", dict(payload_sizes=65280)),
             ("text65536", shapes[:65536], dict(payload_sizes=65536)),
             ("level0", dec, dict(payload_sizes=rnd, level=0)),
             ("fixed", dec, dict(payload_sizes=rnd, strategy=zlib.Z_FIXED)),
             ("huffman_only", dec, dict(payload_sizes=rnd, strategy=zlib.Z_HUFFMAN_ONLY)),
             ("rle", dec, dict(payload_sizes=rnd, strategy=zlib.Z_RLE)),
             ("level1", dec, dict(payload_sizes=rnd, level=1)),
             ("level9", dec, dict(payload_sizes=rnd, level=9)),
             ("flush5000", dec, dict(payload_sizes=rnd, flush_every=5000)),
             ("default", dec, dict(payload_sizes=rnd))]
    return cases


def test_helper_files_are_gzip_files(tmp_path, texts):
    for name, text, kw in _cases(texts):
        path = str(tmp_path / (name + ".gz"))
        _bgzf.write_bgzf(path, text, **kw)
        with gzip.open(path, "rb") as fh:
            assert fh.read() == text, name
    both = _bgzf.bgzf_bytes(b">a\nACGT\n", 3) + _bgzf.bgzf_bytes(b">b\nGG\n", 65280)   # (an end marker in the middle)
    assert gzip.decompress(both) == b">a\nACGT\n>b\nGG\n"


def test_levels_and_strategies_reach_the_three_block_decoders(texts):
    body = texts["decoder"][10000:40000]
    assert _bgzf.first_block_type(_bgzf.member(body, level=0)) == 0
    assert _bgzf.first_block_type(_bgzf.member(body, strategy=zlib.Z_FIXED)) == 1
    assert _bgzf.first_block_type(_bgzf.member(body)) == 2
    # random bytes are stored at the default level too (the member cut out of decoder_fasta()'s first header line)
    rnd = texts["decoder"][_bgzf.RND_AT:_bgzf.RND_AT + _bgzf.RND_LEN]
    assert _bgzf.first_block_type(_bgzf.member(rnd)) == 0
    # a full flush inside a member: more than one block, an empty stored block at a byte border among them
    flushed = _bgzf.deflate_raw(body, flush_every=5000)
    assert flushed.count(b"\x00\x00\xff\xff") >= 5 and zlib.decompress(flushed, -15) == body


def _inflate(exe, path):
    return subprocess.run([exe, "inflate", path], capture_output=True, timeout=120)


def _check_inflates(exe, tmp_path, texts):
    for name, text, kw in _cases(texts):
        path = str(tmp_path / (name + ".gz"))
        _bgzf.write_bgzf(path, text, **kw)
        r = _inflate(exe, path)
        assert r.returncode == 0, (name, r.returncode, r.stderr[-2000:])
        assert r.stdout == text, name
        assert b"budget_broken 0" in r.stderr, (name, r.stderr)


def test_host_program_inflates_every_shape(program, tmp_path, texts):
    _check_inflates(program, tmp_path, texts)


def test_walk_refuses_what_is_not_bgzf(program, tmp_path, texts):
    text = texts["shapes"][:50000]
    good = _bgzf.bgzf_bytes(text, 4096)
    files = {"plain_gzip": gzip.compress(text),
             "plain_member_appended": good + gzip.compress(b"ACGT\n"),
             "fname": _bgzf.member(text[:100]) + _bgzf.member(text[100:300], fname=b"x.fa") + _bgzf.EOF_MARKER,
             "cut": good[:-40],
             "garbage_behind": good + b"\0"}
    for name, data in files.items():
        path = tmp_path / (name + ".gz")
        path.write_bytes(data)
        r = _inflate(program, str(path))
        assert r.returncode == 10, (name, r.returncode, r.stderr)   # refused by the walk
    for name, data, want in (("isize_up", good[:-28 - 4] + (50000 % 4096 + 1).to_bytes(4, "little") + good[-28:], 11),
                             ("crc", good[:-28 - 8] + b"\x01\x02\x03\x04" + good[-28 - 4:], 12)):
        path = tmp_path / (name + ".gz")
        path.write_bytes(data)
        r = _inflate(program, str(path))
        assert r.returncode == want, (name, r.returncode, r.stderr)
    path = tmp_path / "eof_only.gz"
    path.write_bytes(_bgzf.EOF_MARKER)
    r = _inflate(program, str(path))
    assert r.returncode == 0 and r.stdout == b""


FUZZ_TRIALS = 1500


def _fuzz_files(tmp_path, texts):
    """small members of every block kind: stored, fixed, dynamic, several blocks in a member, long matches"""
    dec = texts["decoder"]
    small = dec[9000:9000 + 2500] + b">polyA\n" + b"A" * 700 + b"\n" + dec[:400]
    files = []
    for name, kw in (("dyn", dict(payload_sizes=(700, 0, 1300))), ("fixed", dict(payload_sizes=900, strategy=zlib.Z_FIXED)),
                     ("stored", dict(payload_sizes=800, level=0)), ("flush", dict(payload_sizes=2000, flush_every=300))):
        path = str(tmp_path / f"fuzz_{name}.gz")
        _bgzf.write_bgzf(path, small, **kw)
        files.append(path)
    return files


def _check_fuzz(exe, tmp_path, texts, trials):
    total = {}
    for seed, path in enumerate(_fuzz_files(tmp_path, texts)):
        r = subprocess.run([exe, "fuzz", path, str(seed + 1), str(trials)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (path, r.returncode, r.stderr[-3000:])
        f = r.stdout.split("\n")[0].split()
        got = {f[i]: int(f[i + 1]) for i in range(0, len(f), 2)}
        ctx = (path, r.stdout)
        assert got["trials"] == trials == got["refused"] + got["status"] + got["crc"] + got["same"] + got["prefix"] + got["other"], ctx
        assert got["other"] == 0, ctx            # never another text than the one compressed
        assert got["budget_broken"] == 0, ctx    # every decode within 8 x deflate bytes + 1 steps
        assert got["refused"] > 0 and got["status"] > 0, ctx
        assert got["same"] < trials // 10, ctx   # (flips in bytes without a meaning)
        assert got["prefix"] < trials // 100, ctx  # (a cut that happens to fall between two members)
        for key, v in got.items():
            total[key] = total.get(key, 0) + v
    assert total["crc"] > 0, total               # (stored members: a flipped payload byte is caught by the CRC alone)
    return total


def test_corrupted_members_end_with_a_status(program, tmp_path, texts):
    total = _check_fuzz(program, tmp_path, texts, FUZZ_TRIALS)
    assert total["trials"] == 4 * FUZZ_TRIALS


def test_the_same_under_address_and_undefined_behaviour_sanitizers(program_san, tmp_path, texts):
    """the stand-alone program once more, instrumented: a read or write outside a member's blocks, a shift or an overflow the
    language does not define, stops it with a non-zero exit status"""
    _check_inflates(program_san, tmp_path, {"shapes": texts["shapes"][:200000], "decoder": texts["decoder"]})
    _check_fuzz(program_san, tmp_path, texts, FUZZ_TRIALS)
