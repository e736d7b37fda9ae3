"""BGZF files for the tests of the device inflate route (ntjoin_amd/csrc/bgzf_inflate.h, bgzf.hip), written with Python's zlib:
a chain of gzip members with the extra subfield 'B' 'C' (BSIZE = member size - 1), raw deflate data, CRC-32 and ISIZE -- what
`bgzip` writes -- with the member borders, the compression level and strategy and the blocks inside a member under the test's
control; and the FASTA texts those tests compress."""
import itertools
import random
import struct
import zlib

DEFAULT = zlib.Z_DEFAULT_STRATEGY
MAX_MEMBER = 65536          # BSIZE is 16 bits
_HEAD = 18                  # 12 + the 6 bytes of the BC subfield
_small = {}                 # members of up to 2 bytes of text by (payload, level, strategy): a file of a million of them is a join


def deflate_raw(payload, level=6, strategy=DEFAULT, flush_every=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out = []
    if flush_every:
        for p in range(0, len(payload), flush_every):
            out.append(c.compress(payload[p:p + flush_every]))
            if p + flush_every < len(payload):
                out.append(c.flush(zlib.Z_FULL_FLUSH))   # ends the block at a byte border: an empty stored block follows
    else:
        out.append(c.compress(payload))
    out.append(c.flush())
    return b"".join(out)


def member(payload, level=6, strategy=DEFAULT, flush_every=None, fname=None, isize=None, crc=None):
    """one BGZF member; fname: FLG gets FNAME too (no longer BGZF as the device route reads it); isize / crc: a wrong trailer"""
    key = (bytes(payload), level, strategy)
    plain = flush_every is None and fname is None and isize is None and crc is None
    if plain and len(payload) <= 2 and key in _small:
        return _small[key]
    data = deflate_raw(payload, level, strategy, flush_every)
    name = b"" if fname is None else fname + b"\0"
    total = _HEAD + len(name) + len(data) + 8
    assert total <= MAX_MEMBER, "a member of %d bytes does not fit BSIZE" % total
    flg = 4 | (8 if fname is not None else 0)
    m = (struct.pack("<BBBBIBBH", 0x1f, 0x8b, 8, flg, 0, 0, 0xff, 6) + struct.pack("<BBHH", 66, 67, 2, total - 1) + name + data +
         struct.pack("<II", zlib.crc32(payload) if crc is None else crc, len(payload) if isize is None else isize))
    if plain and len(payload) <= 2:
        _small[key] = m
    return m


EOF_MARKER = member(b"")
assert len(EOF_MARKER) == 28


def split_payloads(data, payload_sizes):
    """the text cut into members' payloads: a number, or a sequence that is cycled (0: an empty member)"""
    sizes = [payload_sizes] if isinstance(payload_sizes, int) else list(payload_sizes)
    assert sizes and max(sizes) > 0 and min(sizes) >= 0
    out, p = [], 0
    for s in itertools.cycle(sizes):
        if p >= len(data):
            break
        out.append(data[p:p + s])
        p += s
    return out


def bgzf_bytes(data, payload_sizes, level=6, strategy=DEFAULT, flush_every=None, eof=True):
    data = bytes(data)
    ms = [member(p, level, strategy, flush_every) for p in split_payloads(data, payload_sizes)]
    if eof:
        ms.append(EOF_MARKER)
    return b"".join(ms)


def write_bgzf(path, data, payload_sizes, level=6, strategy=DEFAULT, flush_every=None, eof=True):
    with open(path, "wb") as fh:
        fh.write(bgzf_bytes(data, payload_sizes, level, strategy, flush_every, eof))
    return path


def first_block_type(member_bytes):
    """BTYPE of the first deflate block of a member written by member(): bits 1-2 of its first deflate byte"""
    xlen = struct.unpack_from("<H", member_bytes, 10)[0]
    return (member_bytes[12 + xlen] >> 1) & 3


# ---- the texts -------------------------------------------------------------------------------------------------------------
def _seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _fasta(recs, width, eol, final_newline):
    out = []
    for hdr, seq in recs:
        out.append(">" + hdr + eol)
        for p in range(0, len(seq), width):
            out.append(seq[p:p + width] + eol)
    text = "".join(out)
    if not final_newline and text.endswith(eol):
        text = text[:-len(eol)]
    return text.encode("latin-1")


def shapes_fasta(seed=3):
    """about 1 MB: CRLF lines, lower case, N runs of 700, IUPAC, a '>' inside a header, empty records, 300 tiny records, no final
    newline"""
    rng = random.Random(seed)
    recs = [("chr1 some comment > with a bracket", _seq(rng, 330_000)),
            ("lower", _seq(rng, 90_000).lower()),
            ("empty", ""),
            ("mixed\tcase", "".join(c.lower() if rng.random() < 0.3 else c for c in _seq(rng, 120_000))),
            ("withN", _seq(rng, 60_000) + "N" * 700 + _seq(rng, 50_000) + "n" * 3 + _seq(rng, 20_000) + "N" * 700 + _seq(rng, 9_000)),
            ("iupac", _seq(rng, 40_000) + "RYKM" + _seq(rng, 40_000) + "-" + _seq(rng, 9_000) + "SWBDHVrykm" + _seq(rng, 5_000)),
            ("empty2", ""),
            ("tiny", "ACGTACGTAC")]
    recs += [(f"frag{i}", _seq(rng, rng.randint(20, 600))) for i in range(300)]
    recs.append(("last", _seq(rng, 130_000)))
    return _fasta(recs, 70, "\r\n", False)


RND_AT, RND_LEN = 5, 3000   # the random bytes of decoder_fasta(): [RND_AT, RND_AT + RND_LEN) of the text, inside its first header line


def decoder_fasta(seed=4):
    """the same kind of text (LF lines) with what drives the decoder to its corners: a first header line that carries 3000 random
    bytes (a member of exactly those is stored, whatever the level), 10 000 x A (distance 1, length 258: the overlapping copy),
    a 40 kB sequence that repeats itself after 32 000 bases (distances near the window's 32 768)"""
    rng = random.Random(seed)
    rnd = bytes(rng.choice([b for b in range(256) if b != 10]) for _ in range(RND_LEN))
    far = _seq(rng, 32_000)
    recs = [("polyA", "A" * 10_000),
            ("far", far + far[:8_000]),
            ("body", _seq(rng, 250_000)),
            ("lower", _seq(rng, 60_000).lower()),
            ("withN", _seq(rng, 30_000) + "N" * 700 + _seq(rng, 30_000)),
            ("empty", ""),
            ("iupac", _seq(rng, 20_000) + "RYKM" + _seq(rng, 20_000))]
    recs += [(f"frag{i}", _seq(rng, rng.randint(20, 600))) for i in range(100)]
    text = b">rnd " + rnd + b"\n" + _seq(rng, 5_000).encode() + b"\n" + _fasta(recs, 70, "\n", True)
    assert text[RND_AT:RND_AT + RND_LEN] == rnd
    return text
