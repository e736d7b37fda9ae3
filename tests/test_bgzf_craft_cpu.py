"""CPU tests of the BGZF inflater on DEFLATE that zlib never writes, and on streams that are wrong in one chosen place
(tests/_deflate_craft.py writes both and checks every one against zlib's inflate as it makes it).

 - the writer's own conditions: every member of the seeded generator is accepted by zlib (no case skipped or retried) and a
   census of the generated set holds; the named cases are a few hundred members of one FASTA; every malformed file is refused by
   Python's gzip where the damage is one gzip can see;
 - the host program of tests/test_bgzf_cpu.py (the decoder of bgzf_inflate.h over plain source, sink and table) inflates the legal
   files to zlib's text and ends every malformed file with the outcome and the BgzfStatus of the table in _deflate_craft.malformed();
 - a second stand-alone program decodes every member through the types the KERNEL hands to the decoder (bgzf_dev_io.h: BgzfDevSrc,
   the aligned-word fetch; BgzfDevSink, the word accumulator; BgzfLdsTab, the lane-interleaved table): the source is a heap block
   padded to a whole word with the member at each of the four byte alignments; the sink a heap block of exactly the text's words
   with the text at each of the four alignments, the bytes around it a marker that must be there afterwards (no lane writes a
   neighbour's byte); the table one interleaved array for 64 lanes, the decode running as lane 0, 1, 31 and 63 and every other
   lane's entries a marker that must be there afterwards.  Status, steps and text must be those of the plain types.  Built twice:
   plain, and with -fsanitize=address,undefined (its own main, no preload of anything)."""
import gzip
import subprocess
import zlib

import pytest

from tests import _deflate_craft as dc
from tests.test_bgzf_cpu import CSRC, _build, _compiler

PROGRAM_DEV = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "bgzf_dev_io.h"
using namespace mxg;

struct Sink {  // the plain sink: a block of exactly ISIZE bytes
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
constexpr unsigned char MARK = 0xA5;
constexpr uint16_t TAB_MARK = 0xBEEF;

static unsigned char *block(size_t n)  // n bytes exactly, at a word border (and more: 16)
{
    void *p = nullptr;
    if (posix_memalign(&p, 16, n ? n : 1) != 0) abort();
    return static_cast<unsigned char *>(p);
}
struct Result {
    uint32_t st = 0, steps = 0;
    std::string text;
};
static Result plain_one(const unsigned char *file, const BgzfMember &m)
{
    unsigned char *in = block(m.in_len), *out = block(m.isize);
    memcpy(in, file + m.in_off, m.in_len);
    BgzfHostSrc src{in, m.in_len};
    Sink sink{out, 0, 0xFFFFFFFFu, crc_tab};
    BgzfHostTab tab;
    Result r;
    r.st = bgzf_inflate_member(src, sink, tab, m.isize, &r.steps);
    if (r.st == BGZF_OK && (sink.crc ^ 0xFFFFFFFFu) != m.crc) r.st = BGZF_CRC;
    if (r.st == BGZF_OK) r.text.assign(reinterpret_cast<const char *>(out), m.isize);
    free(in);
    free(out);
    return r;
}
// the member through the kernel's types: deflate data at byte `sa` of its block, text at byte `da` of its block, tables of `lane`
static Result dev_one(const unsigned char *file, const BgzfMember &m, uint32_t sa, uint32_t da, uint32_t lane, bool *clean)
{
    const size_t sn = (sa + (size_t)m.in_len + 3) & ~(size_t)3, dn = (da + (size_t)m.isize + 3) & ~(size_t)3;
    const size_t tn = (size_t)BGZF_TAB_ELEMS * BGZF_BLOCK;
    unsigned char *in = block(sn), *out = block(dn);
    uint16_t *tabs = reinterpret_cast<uint16_t *>(block(tn * 2));
    memset(in, MARK, sn);
    memset(out, MARK, dn);
    for (size_t i = 0; i < tn; ++i) tabs[i] = TAB_MARK;
    memcpy(in + sa, file + m.in_off, m.in_len);
    Result r;
    {
        BgzfDevSrc src{in + sa, m.in_len};
        BgzfDevSink sink{out + da, crc_tab};
        BgzfLdsTab tab{tabs + 2u * lane};
        r.st = bgzf_inflate_member(src, sink, tab, m.isize, &r.steps);
        if (sink.pend) sink.flush();
        if (r.st == BGZF_OK && (sink.crc ^ 0xFFFFFFFFu) != m.crc) r.st = BGZF_CRC;
    }
    *clean = true;
    for (size_t i = 0; i < dn; ++i)
        if ((i < da || i >= da + m.isize) && out[i] != MARK) *clean = false;
    for (size_t i = 0; i < tn; ++i)
        if ((i / 2) % BGZF_BLOCK != lane && tabs[i] != TAB_MARK) *clean = false;
    if (r.st == BGZF_OK) r.text.assign(reinterpret_cast<const char *>(out + da), m.isize);
    free(in);
    free(out);
    free(tabs);
    return r;
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
// exit status: 0 inflated (the text on stdout); 16 + 16 * outcome + status when the file ends otherwise (outcome 0: refused by the
// walk, 1: a member's status, 2: a member's CRC); 3: the kernel's types and the plain ones disagree, or a marker is gone; 9: steps
int main(int argc, char **argv)
{
    if (argc < 2) return 1;
    for (uint32_t i = 0; i < 256; ++i) crc_tab[i] = bgzf_crc32_entry(i);
    const std::vector<unsigned char> f = slurp(argv[1]);
    unsigned char *file = block(f.size());
    memcpy(file, f.data(), f.size());
    struct Free {
        void *p;
        ~Free() { free(p); }
    } file_freed{file};  // (on every way out: the leak check of the sanitizer build counts too)
    BgzfPlan plan;
    if (!bgzf_plan(file, f.size(), plan)) {
        fprintf(stderr, "outcome 0 status 0\n");
        return 16;
    }
    static const uint32_t lanes[4] = {0, 1, 31, 63};
    std::string text;
    uint64_t decodes = 0;
    for (size_t i = 0; i < plan.members.size(); ++i) {
        const BgzfMember &m = plan.members[i];
        const Result p = plain_one(file, m);
        if ((uint64_t)p.steps > 8ull * m.in_len + 1ull) ++budget_broken;
        if (p.steps > max_steps) max_steps = p.steps;
        for (uint32_t sa = 0; sa < 4; ++sa)
            for (uint32_t da = 0; da < 4; ++da) {
                bool clean = false;
                const uint32_t lane = lanes[(sa + da + (uint32_t)i) & 3u];
                const Result d = dev_one(file, m, sa, da, lane, &clean);
                ++decodes;
                if (d.st != p.st || d.steps != p.steps || d.text != p.text || !clean) {
                    fprintf(stderr, "member %zu source+%u sink+%u lane %u: status %u steps %u (plain: %u, %u) text %s markers %s\n", i, sa, da,
                            lane, d.st, d.steps, p.st, p.steps, d.text == p.text ? "same" : "DIFFERENT", clean ? "kept" : "OVERWRITTEN");
                    return 3;
                }
            }
        if (budget_broken) return 9;
        if (p.st != BGZF_OK) {
            const int outcome = p.st == BGZF_CRC ? 2 : 1;
            fprintf(stderr, "outcome %d status %u member %zu\n", outcome, p.st, i);
            return 16 + 16 * outcome + (int)p.st;
        }
        text += p.text;
    }
    fwrite(text.data(), 1, text.size(), stdout);
    fprintf(stderr, "members %zu decodes %llu steps_max %llu budget_broken %llu\n", plan.members.size(), (unsigned long long)decodes,
            (unsigned long long)max_steps, (unsigned long long)budget_broken);
    return 0;
}
"""

SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _build_dev(d, flags):
    src, exe = d / "bgzf_dev.cpp", d / "bgzf_dev"
    src.write_text(PROGRAM_DEV)
    subprocess.check_call([_compiler(), "-std=c++17", "-Wall", "-Werror", "-I", CSRC, *flags, str(src), "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def plain_program(tmp_path_factory):
    """the program of tests/test_bgzf_cpu.py, as that file builds it"""
    return _build(tmp_path_factory.mktemp("bgzf_host_craft"), ["-O2"])


@pytest.fixture(scope="module", params=["plain", "sanitizers"])
def dev_program(request, tmp_path_factory):
    return _build_dev(tmp_path_factory.mktemp("bgzf_dev_" + request.param), ["-O2"] if request.param == "plain" else SAN)


@pytest.fixture(scope="module")
def generated():
    return dc.legal_members(dc.GENERATOR_SEED, dc.GENERATOR_N, dc.GENERATOR_BIG)


@pytest.fixture(scope="module")
def legal_files(tmp_path_factory, generated):
    """{name: (path, text)}: the named cases at the four alignments of the text, the end-of-block-only set, the generator's file"""
    d = tmp_path_factory.mktemp("craft_legal")
    sets = {"named%d" % shift: dc.named_members(shift) for shift in range(4)}
    sets["eob_only"] = dc.named_members(0)[:1] + dc.case_eob_only()
    sets["generated"] = generated[0]
    out = {}
    for name, members in sets.items():
        data, text, _ = dc.file_of(members)
        path = d / (name + ".fa.gz")
        path.write_bytes(data)
        out[name] = (str(path), text)
    return out


@pytest.fixture(scope="module")
def bad_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("craft_bad")
    out = {}
    for name, (data, outcome, status) in dc.malformed().items():
        path = d / (name + ".fa.gz")
        path.write_bytes(data)
        out[name] = (str(path), outcome, status)
    return out


def test_every_generated_member_is_accepted_by_zlib_and_the_census_holds(generated):
    members, census = generated           # (legal_members asserts zlib's text for every member as it makes it: none is skipped)
    assert len(members) == dc.GENERATOR_N + dc.GENERATOR_BIG
    for m, text in members:
        assert gzip.decompress(m) == text and dc.is_fasta(text)
    sizes = sorted(len(t) for _, t in members)
    assert sizes[dc.GENERATOR_N - 1] <= 4096 and sizes[dc.GENERATOR_N] >= 40000 and sizes[-1] <= 65536
    for key in dc.CENSUS_KEYS:
        assert census[key] >= 1, (key, census)
    again, _ = dc.legal_members(dc.GENERATOR_SEED, 0, 1)
    assert again[0] == members[0]                                        # seeded: the same file every time


def test_named_cases_are_one_fasta_of_a_few_hundred_members():
    firsts = set()
    for shift in range(4):
        members = dc.named_members(shift)
        data, text, n = dc.file_of(members)
        assert 300 < n == len(members) < 500 and len(data) < len(text)
        assert max(len(t) for _, t in members) == 65536
        assert sum(1 for _, t in members if len(t) < 300) > 300             # most are tiny
        firsts.add(len(members[0][1]) % 4)
    assert firsts == {0, 1, 2, 3}                                            # every later member at each alignment of the text


def test_malformed_files_are_refused_by_gzip_where_gzip_can_see_it():
    table = dc.malformed()
    assert len(table) == 44 and max(len(data) for data, _, _ in table.values()) < 400
    for name, (data, outcome, status) in table.items():
        if outcome == dc.REFUSED and name != "isize_65537":      # (an odd extra field is gzip's to skip: legal gzip, not BGZF)
            assert gzip.decompress(data) == b">bad\nACGTACGTAC\n", name
            continue
        with pytest.raises((OSError, EOFError, zlib.error)):
            gzip.decompress(data)
        assert (outcome == dc.REFUSED) == (status == dc.OK), name


def _run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, timeout=300)


def test_plain_types_inflate_the_legal_files(plain_program, legal_files):
    for name, (path, text) in legal_files.items():
        r = _run(plain_program, "inflate", path)
        assert r.returncode == 0, (name, r.returncode, r.stderr[-2000:])
        assert r.stdout == text, name
        assert b"budget_broken 0" in r.stderr, (name, r.stderr)


def test_plain_types_end_the_malformed_files_as_the_table_says(plain_program, bad_files):
    for name, (path, outcome, status) in bad_files.items():
        r = _run(plain_program, "inflate", path)
        assert r.returncode == 10 + outcome, (name, r.returncode, r.stderr[-2000:])
        assert r.stderr.decode().startswith("outcome %d status %d\n" % (outcome, status)), (name, r.stderr)


def test_kernel_types_inflate_the_legal_files(dev_program, legal_files):
    for name, (path, text) in legal_files.items():
        r = _run(dev_program, path)
        assert r.returncode == 0, (name, r.returncode, r.stderr[-3000:])
        assert r.stdout == text, name
        assert b"budget_broken 0" in r.stderr, (name, r.stderr)


def test_kernel_types_end_the_malformed_files_as_the_plain_types_do(dev_program, bad_files):
    for name, (path, outcome, status) in bad_files.items():
        r = _run(dev_program, path)
        assert r.returncode == 16 + 16 * outcome + status, (name, r.returncode, r.stderr[-3000:])   # (3: the types disagree; 9: steps)
        assert r.stderr.decode().startswith("outcome %d status %d" % (outcome, status)), (name, r.stderr)
        assert r.stdout == b""
