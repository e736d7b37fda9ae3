"""CPU tests of the BGZF member coder the device writer compiles into its kernel (ntjoin_amd/csrc/bgzf_deflate.h), built into a small
host program (tests/_bgzf_deflate_host.py) as tests/test_bgzf_cpu.py builds the decoder's.

For every payload kind -- no text, 1 and 2 bytes, one byte value 65 280 times, i.i.d. ACGT, the FASTA shapes of tests/_bgzf.py cut
at 65 280 and at 1000 bytes, all 256 byte values, random bytes (which must come out stored), 22 symbols with Fibonacci counts,
18 symbols whose Huffman tree is one chain (deeper than 15 whatever the ties: the length limit) --
 - gzip.decompress of the file gives the text (Python checks CRC-32 and ISIZE of every member);
 - BSIZE walks the file exactly to its end, the last 28 bytes are the end marker, no member is larger than its text + 31;
 - this repository's own bgzf_plan + bgzf_inflate_member accept every member and give the text (the program does that itself);
 - a member is no larger than 18 + 8 + zlib's Z_HUFFMAN_ONLY raw deflate of the same payload + 64 bytes: an optimal limited code
   gives both coders the same data bits; what may differ is the block header and zlib's choice of block type and block borders;
 - the same program built with -fsanitize=address,undefined (its own main, no preload) repeats the run: source and sink are heap
   blocks of exact size."""
import gzip
import random
import struct
import zlib

import pytest

from tests import _bgzf, _bgzf_deflate_host as host

P_MAX = 65280


def fibonacci_text():
    "22 symbols with counts 1, 1, 2, 3, 5, ...: 46 367 bytes, shuffled"
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    text = bytearray()
    for s, c in enumerate(fib):
        text += bytes([65 + s]) * c
    assert len(text) == 46367
    random.Random(11).shuffle(text)
    return bytes(text)


def deep_counts():
    """counts of 18 literals for which the Huffman tree of literals + end-of-block code (count 1) is one chain whatever the ties:
    every literal is more frequent than the tree merged so far and than the literal before it"""
    counts = [2, 3]
    while len(counts) < 18:
        counts.append(2 + sum(counts[:-1]))   # one more than the tree of the end-of-block code and all literals but the last
    return counts


def deep_text():
    "the length limit at work: a code of depth 18 without the limit, in one block of a member (under 32 640 bytes), shuffled"
    text = bytearray()
    for s, c in enumerate(deep_counts()):
        text += bytes([97 + s]) * c
    assert len(text) < 32640
    random.Random(12).shuffle(text)
    return bytes(text)


def huffman_depth(counts):
    nodes = sorted((c, 0) for c in counts)   # (weight, depth of the deepest leaf below)
    while len(nodes) > 1:
        (wa, da), (wb, db) = nodes[0], nodes[1]
        nodes = sorted(nodes[2:] + [(wa + wb, max(da, db) + 1)])
    return nodes[0][1]


def payload_kinds():
    "(name, text, bytes of text per member)"
    rng = random.Random(7)
    shapes = _bgzf.shapes_fasta()
    return [("empty", b"", P_MAX),
            ("one", b"A", P_MAX),
            ("two", b"AC", P_MAX),
            ("same", b"N" * P_MAX, P_MAX),
            ("acgt", bytes(rng.choice(b"ACGT") for _ in range(P_MAX)), P_MAX),
            ("shapes", shapes, P_MAX),
            ("shapes1000", shapes[:200_000], 1000),
            ("all256", bytes(range(256)), P_MAX),
            ("random", rng.randbytes(P_MAX), P_MAX),
            ("fibonacci", fibonacci_text(), P_MAX),
            ("deep", deep_text(), P_MAX)]


def walk(data):
    "the members of a BGZF file as (offset, size), by BSIZE; asserts the fixed header bytes"
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 10:at + 16] == b"\x06\x00BC\x02\x00", at
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        out.append((at, size))
        at += size
    assert at == len(data)
    return out


def check_file(data, text, payload, name=""):
    "everything the tests ask of a BGZF file of `text` at `payload` bytes per member; returns how many members are stored"
    assert gzip.decompress(data) == text, name
    members = walk(data)
    assert data[-28:] == _bgzf.EOF_MARKER, name
    assert len(members) == (len(text) + payload - 1) // payload + 1, name
    stored = 0
    for j, (at, size) in enumerate(members[:-1]):
        p = text[j * payload:(j + 1) * payload]
        assert size <= len(p) + 31, (name, j)
        assert struct.unpack_from("<II", data, at + size - 8) == (zlib.crc32(p), len(p)), (name, j)
        cap = 18 + 8 + len(_bgzf.deflate_raw(p, 6, zlib.Z_HUFFMAN_ONLY)) + 64
        assert size <= cap, (name, j, size, cap)
        btype = (data[at + 18] >> 1) & 3
        assert btype in (0, 2) and (btype == 2 or data[at + 18] & 1), (name, j)   # dynamic blocks, or one final stored block
        stored += btype == 0
    return stored


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host.build(tmp_path_factory.mktemp("bgzf_deflate_host"), ["-O2"])


@pytest.fixture(scope="module")
def program_san(tmp_path_factory):
    return host.build(tmp_path_factory.mktemp("bgzf_deflate_host_san"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run_all(exe, tmp_path):
    for name, text, payload in payload_kinds():
        data, info = host.deflate(exe, payload, text, tmp_path, name)
        stored = check_file(data, text, payload, name)
        assert info == {"members": (len(text) + payload - 1) // payload, "stored": stored, "bytes_in": len(text), "bytes_out": len(data)}, name
        if name == "empty":
            assert data == _bgzf.EOF_MARKER
        if name == "random":
            assert stored == 1
        if name in ("acgt", "same", "fibonacci", "shapes", "deep"):
            assert stored == 0, name
        if name == "acgt":
            assert len(data) < 0.29 * len(text)      # 2 bits a base and a header of tens of bytes
        if name == "same":
            assert len(data) < len(text) / 8 + 100   # 1 bit a base: no match search


def test_every_payload_kind(program, tmp_path):
    _run_all(program, tmp_path)


def test_the_length_limit_is_reached():
    """the `deep` text needs the limit of 15 bits whatever the ties are broken by.  (The Fibonacci text of 22 symbols does so only
    without the end-of-block code: with its count of 1 beside the two literals of count 1, a Huffman tree of depth 12 exists.)"""
    assert huffman_depth(deep_counts() + [1]) > 15
    text = deep_text()
    assert huffman_depth([text.count(bytes([97 + s])) for s in range(18)] + [1]) > 15


def test_member_borders_depend_on_the_payload_size_only(program, tmp_path):
    text = _bgzf.shapes_fasta()[:150_000]
    for payload in (1, 7, 255, 256, 4096):
        t = text[:20_000]
        data, info = host.deflate(program, payload, t, tmp_path, f"p{payload}")
        check_file(data, t, payload, f"p{payload}")
    whole, _ = host.deflate(program, 1000, text, tmp_path, "whole")
    head, _ = host.deflate(program, 1000, text[:64_000], tmp_path, "head")
    assert whole[:len(head) - 28] == head[:-28]   # a prefix of whole members is the same bytes


def test_the_same_under_address_and_undefined_behaviour_sanitizers(program_san, tmp_path):
    _run_all(program_san, tmp_path)
