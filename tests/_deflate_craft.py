"""A DEFLATE writer under the test's control, for the BGZF inflater (ntjoin_amd/csrc/bgzf_inflate.h, bgzf_dev_io.h, bgzf.hip): the
streams zlib's deflate never writes but its inflate accepts -- distances up to 32 768, length 258 as 284 + 31, codes of 15 bits,
a distance set of one code, every corner of the code-length header -- and streams that are wrong in one chosen place.

Plain Python: an LSB-first bit writer, canonical codes from explicit length lists, block writers over a token list (a literal byte,
or (length, distance[, True: spell 258 as 284 + 31])).  The rules of this file:
 - every legal raw stream is checked WHEN IT IS MADE: zlib.decompress(raw, -15) == the text its tokens spell (Stream.legal);
 - every malformed stream is checked when it is made to raise zlib.error (Stream.bad), and where the damage is in the sizes or the
   trailer the whole member is checked to fail through gzip.decompress (bad_member);
 - every text is a FASTA the ingest accepts (is_fasta): it starts with '>', header bytes are anything but a line feed, sequence
   lines are plain letters.
zlib's inflate is the reference; the code under test never is."""
import bisect
import collections
import gzip
import random
import struct
import zlib

from tests import _bgzf

ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)   # the code-length code's lengths come in this order
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]    # symbols 257 .. 285
LEN_BASE = []
_b = 3
for _e in LEN_EXTRA[:-1]:
    LEN_BASE.append(_b)
    _b += 1 << _e
LEN_BASE.append(258)
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]         # symbols 0 .. 29
DIST_BASE = []
_b = 1
for _e in DIST_EXTRA:
    DIST_BASE.append(_b)
    _b += 1 << _e
assert LEN_BASE[:9] == [3, 4, 5, 6, 7, 8, 9, 10, 11] and LEN_BASE[27] == 227 and DIST_BASE[29] == 24577 and _b == 32769
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DL = [5] * 32
SEQ = b"ACGTNacgtn"
FAR = 32507                     # zlib's deflate never looks further back than 32 768 - 262 = 32 506


_REVERSED = {}


class BitWriter:
    def __init__(self):
        self.buf, self.acc, self.n = bytearray(), 0, 0

    def pos(self):
        return 8 * len(self.buf) + self.n

    def bits(self, value, n):
        """n bits of a number, least significant first"""
        assert 0 <= value < (1 << n) or n == 0 and value == 0
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        """a Huffman code: most significant bit first"""
        rev = _REVERSED.get((code, n))
        if rev is None:
            rev = _REVERSED[code, n] = int(format(code, "0%db" % n)[::-1], 2)
        self.bits(rev, n)

    def align(self, ones=False):
        if self.n:
            k = 8 - self.n
            self.bits((1 << k) - 1 if ones else 0, k)

    def done(self):
        self.align()
        return bytes(self.buf)


def canonical(lengths):
    """{symbol: (code, bits)} of the canonical code of a list of lengths (RFC 1951, 3.2.2)"""
    count = collections.Counter(l for l in lengths if l)
    code, nxt = 0, {}
    for b in range(1, 16):
        code = (code + count.get(b - 1, 0)) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l] & ((1 << l) - 1), l)   # (an over-subscribed set, made on purpose, wraps: nothing decodes it anyway)
            nxt[l] += 1
    return out


def kraft(lengths):
    """the code space a set uses, in units of 2^-15: 32768 = complete"""
    return sum(32768 >> l for l in lengths if l)


def len_code(length, alt=False):
    if length == 258 and not alt:
        return 285, 0, 0
    s = bisect.bisect_right(LEN_BASE, length, 0, 28) - 1
    assert length - LEN_BASE[s] < (1 << LEN_EXTRA[s])
    return 257 + s, LEN_EXTRA[s], length - LEN_BASE[s]


def dist_code(dist):
    s = bisect.bisect_right(DIST_BASE, dist) - 1
    assert dist - DIST_BASE[s] < (1 << DIST_EXTRA[s])
    return s, DIST_EXTRA[s], dist - DIST_BASE[s]


def apply(tokens, text=b""):
    """the text a token list spells behind `text`"""
    out = bytearray(text)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            assert 3 <= t[0] <= 258 and 1 <= t[1] <= len(out), t
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out[len(text):])


def used_symbols(tokens):
    """(literal/length symbols with the end-of-block code, distance symbols) a token list needs"""
    ls, ds = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            ls.add(t)
        else:
            ls.add(len_code(t[0], len(t) > 2 and t[2])[0])
            ds.add(dist_code(t[1])[0])
    return ls, ds


def tree_lengths(n, rng, maxbits=15, deep=0.5):
    """the leaf depths of a random full binary tree with n leaves: Kraft-complete and depth-limited by construction"""
    if n == 1:
        return [1]
    assert n <= (1 << maxbits)
    leaves, deepest = [0], 0   # deepest: a leaf of the greatest depth below maxbits
    while len(leaves) < n:
        i = deepest
        if rng.random() >= deep:
            i = rng.randrange(len(leaves))
            while leaves[i] >= maxbits:
                i = rng.randrange(len(leaves))
        d = leaves[i] + 1
        leaves[i] = d
        leaves.append(d)
        if d >= maxbits and i == deepest:
            deepest = max((j for j, e in enumerate(leaves) if e < maxbits), key=lambda j: leaves[j], default=0)
        elif d < maxbits and d > leaves[deepest]:
            deepest = i
    rng.shuffle(leaves)
    return leaves


def set_from(symbols, n, rng, maxbits=15, deep=0.5, weights=None):
    """n lengths: a random complete code over `symbols`, 0 elsewhere; weights: the shorter codes go to the heavier symbols"""
    symbols = sorted(symbols)
    lengths = tree_lengths(len(symbols), rng, maxbits, deep)
    if weights is not None:
        symbols.sort(key=lambda s: -weights.get(s, 0))
        lengths.sort()
    out = [0] * n
    for s, l in zip(symbols, lengths):
        out[s] = l
    return out


def fit_lengths(n, forced, text_syms, spare):
    """n lengths of a complete code: `forced` {symbol: length} as given, the text's other symbols share what is left at one length,
    and symbols of `spare` (no text uses them) take the remainder, one per binary digit"""
    out = [0] * n
    for s, l in forced.items():
        out[s] = l
    left = 32768 - kraft(out)
    todo = [s for s in sorted(text_syms) if not out[s]]
    if todo:
        t = 1
        while len(todo) * (32768 >> t) > left:
            t += 1
        assert t <= 15
        for s in todo:
            out[s] = t
        left -= len(todo) * (32768 >> t)
    sp = [s for s in spare if not out[s]]
    for l in range(1, 16):
        if left & (32768 >> l):
            out[sp.pop(0)] = l
            left -= 32768 >> l
    assert left == 0 and kraft(out) == 32768
    return out


def cl_rle(lengths, rng=None):
    """the code-length symbols of a list of lengths: a length, or (16 | 17 | 18, repeat).  Without rng every run is taken as long
    as the format allows; with one, a random legal choice."""
    out, i, n = [], 0, len(lengths)
    while i < n:
        v, j = lengths[i], i
        while j < n and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3 and (rng is None or rng.random() < 0.8):
            rep = min(run, 138) if rng is None or rng.random() < 0.3 else rng.randint(3, min(run, 138))
            out.append((18 if rep >= 11 else 17, rep))
        elif i > 0 and lengths[i - 1] == v and run >= 3 and (rng is None or rng.random() < 0.7):
            rep = min(run, 6) if rng is None or rng.random() < 0.3 else rng.randint(3, min(run, 6))
            out.append((16, rep))
        else:
            rep = 1
            out.append(v)
        i += rep
    return out


def cl_expand(seq):
    out = []
    for t in seq:
        if isinstance(t, int):
            out.append(t)
        elif t[0] == 16:
            out += [out[-1]] * t[1]
        else:
            out += [0] * t[1]
    return out


def cl_code_lengths(seq, rng=None):
    """19 lengths of a complete code-length code over the symbols a sequence uses (the code-length code may not be incomplete: one
    used symbol gets an unused partner)"""
    used = sorted({t if isinstance(t, int) else t[0] for t in seq})
    if len(used) == 1:
        used.append(0 if used[0] else 1)
    if rng is None:
        k = len(used).bit_length() - 1
        short = (2 << k) - len(used)
        ls = [k] * short + [k + 1] * (len(used) - short)
    else:
        ls = tree_lengths(len(used), rng, 7, 0.3)
    out = [0] * 19
    for s, l in zip(sorted(used), ls):
        out[s] = l
    assert kraft(out) == 32768 and max(out) <= 7
    return out


class Stream:
    """one raw DEFLATE stream, block by block; .text is what it spells, .census what it used"""

    def __init__(self):
        self.w, self.text, self.blocks = BitWriter(), bytearray(), []
        self.census = collections.Counter()

    def _head(self, last, kind):
        self.w.bits(1 if last else 0, 1)
        self.w.bits(kind, 2)
        self.blocks.append(kind)
        self.census["type%d" % kind] += 1

    def stored(self, data, last=False, ones=False, nlen=None, length=None):
        self._head(last, 0)
        self.w.align(ones)
        n = len(data) if length is None else length
        self.w.buf += struct.pack("<HH", n, (n ^ 0xFFFF) if nlen is None else nlen) + bytes(data)
        self.text += data
        return self

    def fixed(self, tokens, last=False, eob=True):
        self._head(last, 1)
        lc, dc = canonical(FIXED_LL), canonical(FIXED_DL)
        self.tokens(tokens, lc, dc)
        if eob:
            self.w.code(*lc[256])
        return self

    def dynamic(self, tokens, ll, dl, last=False, hclen=None, cl_seq=None, cl_lens=None, eob=True, strict=True):
        """ll, dl: the lengths of both sets (HLIT = len(ll), HDIST = len(dl)); cl_seq: the exact code-length symbols (cl_rle's by
        default); cl_lens: the 19 lengths of the code-length code; hclen: how many of them are sent (the fewest by default);
        strict=False: a header that is wrong on purpose"""
        lens = list(ll) + list(dl)
        if cl_seq is None:
            cl_seq = cl_rle(lens)
        if cl_lens is None:
            cl_lens = cl_code_lengths(cl_seq)
        need = max([i for i, s in enumerate(ORDER) if cl_lens[s]] + [0]) + 1
        if hclen is None:
            hclen = max(4, need)
        if strict:
            assert 257 <= len(ll) <= 286 and 1 <= len(dl) <= 30 and cl_expand(cl_seq) == lens and need <= hclen <= 19
            assert kraft(cl_lens) == 32768 and ll[256]
        self._head(last, 2)
        self.cl_seq = list(cl_seq)
        w = self.w
        w.bits(len(ll) - 257, 5)
        w.bits(len(dl) - 1, 5)
        w.bits(hclen - 4, 4)
        for i in range(hclen):
            w.bits(cl_lens[ORDER[i]], 3)
        cc = canonical(cl_lens)
        for t in cl_seq:
            if isinstance(t, int):
                w.code(*cc[t])
            else:
                w.code(*cc[t[0]])
                w.bits(t[1] - (11 if t[0] == 18 else 3), {16: 2, 17: 3, 18: 7}[t[0]])
        lc, dc = canonical(ll), canonical(dl)
        self.census["hclen_below_19"] += hclen < 19
        self.census["hclen_%d" % hclen] += 1
        for t in cl_seq:
            if not isinstance(t, int):
                self.census["cl%d" % t[0]] += 1
        single = sum(1 for l in dl if l) == 1
        before = self.census["matches"]
        self.tokens(tokens, lc, dc)
        self.census["single_distance_code"] += single and self.census["matches"] > before
        if eob:
            w.code(*lc[256])
        return self

    def tokens(self, tokens, lc, dc):
        """the codes of a token list.  Beside literals and matches: ("L", s) a bare literal/length symbol, ("D", s) a bare distance
        symbol, ("B", value, n) n plain bits -- for streams that are wrong on purpose."""
        w, c = self.w, self.census
        for t in tokens:
            if isinstance(t, int):
                w.code(*lc[t])
                c["bits15"] += lc[t][1] == 15
                self.text.append(t)
            elif t[0] == "L":
                w.code(*lc[t[1]])
            elif t[0] == "D":
                w.code(*dc[t[1]])
            elif t[0] == "B":
                w.bits(t[1], t[2])
            else:
                ls, leb, lev = len_code(t[0], len(t) > 2 and t[2])
                w.code(*lc[ls])
                w.bits(lev, leb)
                ds, deb, dev = dist_code(t[1])
                w.code(*dc[ds])
                w.bits(dev, deb)
                c["bits15"] += (lc[ls][1] == 15) + (dc[ds][1] == 15)
                c["matches"] += 1
                c["far"] += t[1] >= FAR
                c["overlap"] += t[1] < t[0]
                c["len_%d_%d" % (ls, lev)] += 1
                c["dist_%d_lo" % ds] += dev == 0
                c["dist_%d_hi" % ds] += dev == (1 << deb) - 1
                c["dist_%d_mid" % ds] += 0 < dev < (1 << deb) - 1
                if t[1] <= len(self.text):   # (else: wrong on purpose)
                    for _ in range(t[0]):
                        self.text.append(self.text[-t[1]])

    def legal(self):
        raw = self.w.done()
        assert zlib.decompress(raw, -15) == bytes(self.text), "the writer is wrong"
        return raw

    def bad(self, cut=None):
        """the raw bytes (the first `cut` of them) of a stream zlib refuses"""
        raw = self.w.done()[:cut]
        try:
            zlib.decompress(raw, -15)
        except zlib.error:
            return raw
        raise AssertionError("zlib takes the stream that was meant to be wrong")


def member(raw, text, before=(), after=(), isize=None, crc=None, subfields=None, stray=b""):
    """a BGZF member around raw deflate data, like _bgzf.member: extra subfields (two-letter id, bytes) before and after 'BC'.
    subfields: the whole list instead, where the bytes None stand for BSIZE and a number n for BSIZE followed by n more bytes;
    stray: bytes behind the last subfield, inside XLEN"""
    if subfields is None:
        subfields = list(before) + [(b"BC", None)] + list(after)
    xlen = sum(4 + (2 if d is None else 2 + d if isinstance(d, int) else len(d)) for _, d in subfields) + len(stray)
    total = 12 + xlen + len(raw) + 8
    assert total <= 65536 and xlen < 65536
    extra = b""
    for ident, d in subfields:
        data = struct.pack("<H", total - 1) + (b"" if d is None else bytes(d)) if d is None or isinstance(d, int) else bytes(d)
        extra += ident + struct.pack("<H", len(data)) + data
    extra += stray
    assert len(extra) == xlen
    return (struct.pack("<BBBBIBBH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, xlen) + extra + raw +
            struct.pack("<II", zlib.crc32(text) if crc is None else crc, len(text) if isize is None else isize))


def good_member(stream, **kw):
    text = bytes(stream.text)
    m = member(stream.legal(), text, **kw)
    assert gzip.decompress(m) == text
    return m


def bad_member(raw, text, **kw):
    """a member whose deflate data is legal but whose sizes or trailer are not: gzip.decompress must refuse it"""
    m = member(raw, text, **kw)
    try:
        gzip.decompress(m)
    except (OSError, EOFError, zlib.error):
        return m
    raise AssertionError("gzip takes the member that was meant to be wrong")


def is_fasta(text):
    if not text.startswith(b">"):
        return False
    ok = set(SEQ)
    return all(line.startswith(b">") or set(line) <= ok for line in text.split(b"\n"))


def file_of(members, eof=True):
    """(file bytes, text, number of non-empty members) of a list of (member bytes, text)"""
    data = b"".join(m for m, _ in members) + (_bgzf.EOF_MARKER if eof else b"")
    text = b"".join(t for _, t in members)
    assert is_fasta(text) and gzip.decompress(data) == text
    return data, text, sum(1 for _, t in members if t)


def _seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choices(alphabet, k=n))


def _auto_dynamic(stream, tokens, rng, last=True, deep=0.5, **kw):
    """a dynamic block whose sets are random complete codes over exactly what the tokens use"""
    ls, ds = used_symbols(tokens)
    if len(ls) == 1:
        ls.add(65)
    ll = set_from(ls, max(257, max(ls) + 1), rng, 15, deep)
    dl = set_from(ds, max(ds) + 1, rng, 15, deep) if ds else [0]
    return stream.dynamic(tokens, ll, dl, last, **kw)


# ---- the named legal cases ----------------------------------------------------------------------------------------------------
def _m(stream, **kw):
    return good_member(stream, **kw), bytes(stream.text)


def _lits(b):
    return list(b)


def case_deep():
    """lengths 1, 2, ..., 14, 15, 15 in both sets; the 15-bit codes on a literal, a length symbol and a distance symbol in use"""
    order = [65, 67, 71, 84, 10, 256, 62, 100, 101, 112, 97, 99, 103, 116, 78, 260]    # A C G T \n EOB > d e p a c g t | N, length 6
    ll = [0] * 261
    for i, s in enumerate(order):
        ll[s] = min(i + 1, 15)
    dl = [min(i + 1, 15) for i in range(16)]                                            # symbols 14 and 15: 15 bits
    body = b"ACGTNacgt" * 20
    tokens = _lits(b">deep\n" + body) + [(6, 150), 78, (6, 1), (6, 193), 10]            # distance symbols 14, 0, 15
    s = Stream().dynamic(tokens, ll, dl, True, hclen=19)
    assert s.census["bits15"] >= 4 and s.census["hclen_19"] == 1 and s.census["dist_14_mid"] and s.census["dist_15_lo"]
    return [_m(s)]


def _length_tokens():
    out = _lits(b"ACGTACGT")
    for s in range(28):
        out += [(LEN_BASE[s], 4), (LEN_BASE[s] + (1 << LEN_EXTRA[s]) - 1, 4)]
    return out + [(258, 4), (258, 4, True), (257, 4), 10]    # 285; 284 + 31; 284 + 30


def case_lengths(rng):
    """every length symbol at its smallest and largest extra bits, 284 + 30 and 284 + 31: once dynamic, once fixed"""
    a = _auto_dynamic(Stream(), _lits(b">lengths\n") + _length_tokens(), rng)
    b = Stream().fixed(_lits(b">lengths_fixed\n") + _length_tokens(), True)
    for s in (a, b):
        for sym in range(257, 285):
            e = LEN_EXTRA[sym - 257]
            assert s.census["len_%d_0" % sym] and s.census["len_%d_%d" % (sym, (1 << e) - 1)], sym
        assert s.census["len_285_0"] and s.census["len_284_31"] and s.census["len_284_30"]
    return [_m(a), _m(b)]


def case_far(rng):
    """32 768 bytes of sequence, then: a match with dist == out from the member's first byte, every distance symbol at its smallest
    and largest extra bits (32 768 among them), several distances from 32 507 on"""
    head = Stream().stored(b">far\n", True)
    tokens = _lits(_seq(rng, 32768)) + [(10, 32768)]
    for d in range(30):
        tokens += [(3 + d % 5, DIST_BASE[d]), (3 + (d + 1) % 5, DIST_BASE[d] + (1 << DIST_EXTRA[d]) - 1)]
    tokens += [(258, 32768), (4, FAR), (5, 32600), (3, 32767), (257, 32768, False), 10]
    s = _auto_dynamic(Stream(), tokens, rng, deep=0.2)
    for d in range(30):
        assert s.census["dist_%d_lo" % d] and s.census["dist_%d_hi" % d], d
    assert s.census["far"] >= 6 and len(s.text) > 32768 + 258
    t = Stream().fixed(_lits(_seq(rng, 32768)) + [(9, 32768), (3, 24577), (3, 32768), (7, FAR + 1), 10], True)
    return [_m(head), _m(s), _m(t)]


def case_overlaps(rng):
    """distance 1 .. 8 x length 3 .. 12 and 258 with 0 .. 3 literals in front of the distance's own: one tiny member each"""
    out = [_m(Stream().stored(b">overlaps\n", True))]
    i = 0
    for dist in range(1, 9):
        for length in list(range(3, 13)) + [258]:
            for front in range(4):
                tokens = _lits(_seq(rng, front + dist)) + [(length, dist), 10]
                s = Stream().fixed(tokens, True) if i % 2 else _auto_dynamic(Stream(), tokens, rng)
                out.append(_m(s))
                i += 1
    assert i == 8 * 11 * 4
    return out


SPARE = list(range(11, 32))   # control characters no text of the header cases uses: they take what a set has left


def _corner(name, forced, rng, nlen=257, dl=(0,), matches=(), **kw):
    tokens = _lits(b">" + name.encode() + b"\n" + _seq(rng, 40)) + list(matches) + [10]
    ls, _ = used_symbols(tokens)
    ll = fit_lengths(max(nlen, max(ls) + 1), forced, ls, SPARE)
    return Stream().dynamic(tokens, ll, list(dl), True, **kw)


def case_headers(rng):
    out = []
    # HCLEN 5: the lengths 16 17 18 0 8 -- every code has 8 bits (HCLEN 4 sends only 16 17 18 0: no length but 0 can be said, so no
    # legal block has it; MALFORMED holds that one)
    tokens = _lits(b">hclen5\n" + _seq(rng, 30) + b"\n")
    s = Stream().dynamic(tokens, [0] + [8] * 256, [0], True, cl_seq=[0] + [8] * 256 + [0], cl_lens=[1 if i in (0, 8) else 0 for i in range(19)])
    assert s.census["hclen_5"] == 1
    out.append(_m(s))
    # HLIT 257 and HDIST 1; 17 x 10 (bytes 0 .. 9) and 18 x 138 (bytes 118 .. 255: no letter behind 'u')
    s = _corner("hlit257", {}, rng)
    assert (17, 10) in s.cl_seq and (18, 138) in s.cl_seq and len(cl_expand(s.cl_seq)) == 257 + 1
    out.append(_m(s))
    # HLIT 286 and HDIST 30: the last symbol of either set has a length, and is used
    s = _corner("hlit286", {285: 9}, rng, nlen=286, dl=[5] * 28 + [4, 4], matches=[(258, 30), (3, 1)])
    out.append(_m(s))
    # 16 at index 1; 16 copying a 15
    s = _corner("c16at1", {0: 9, 1: 9, 2: 9, 3: 9}, rng)
    assert s.cl_seq[:2] == [9, (16, 3)]
    out.append(_m(s))
    s = _corner("c16of15", {b: 15 for b in range(200, 207)}, rng)
    out.append(_m(s))
    assert any(a == 15 and b == (16, 6) for a, b in zip(s.cl_seq, s.cl_seq[1:]))
    # a repeat that ends exactly at nlen + ndist (2, 16 x 3); a non-zero 16 that runs from the literal lengths into the distances
    s = _corner("endrep", {}, rng, dl=[2, 2, 2, 2], matches=[(5, 3), (4, 4)])
    assert s.cl_seq[-2:] == [2, (16, 3)]
    out.append(_m(s))
    s = _corner("cross", {284: 4, 285: 4}, rng, nlen=286, dl=[4] * 16, matches=[(240, 20), (258, 33), (3, 200)])
    assert s.cl_seq[-4:] == [4, (16, 6), (16, 6), (16, 5)]    # (285 and five distance lengths in one repeat; the last ends at the total)
    out.append(_m(s))
    # HCLEN 19 with 18 x 138 and the longest zero runs, random choices of 16 17 18 over the same sets
    for i in range(4):
        tokens = _lits(b">rnd%d\n" % i + _seq(rng, 50)) + [(20, 7), (3, 50), 10]
        ls, ds = used_symbols(tokens)
        ll = set_from(ls | set(range(130, 130 + 3 * i)), 286, rng)
        dl = set_from(ds | {29}, 30, rng)
        seq = cl_rle(ll + dl, rng)
        out.append(_m(Stream().dynamic(tokens, ll, dl, True, cl_seq=seq, cl_lens=cl_code_lengths(seq, rng), hclen=19)))
    return out


def case_special_sets(rng):
    out = []
    # one distance code of one bit: HDIST 1, and the same code on distance symbol 2 (HDIST 3)
    body = _lits(b">single\nACGTTGCA")
    for tokens, dl in ((body + [(8, 1), (30, 1), 10], [1]), (body + [(8, 3), (258, 3), 10], [0, 0, 1])):
        ls = used_symbols(tokens)[0]
        s = Stream().dynamic(tokens, fit_lengths(max(ls) + 1, {}, ls, SPARE), dl, True)
        assert s.census["single_distance_code"] == 1
        out.append(_m(s))
    # no distance code: literals only
    out.append(_m(_corner("literals", {}, rng)))
    return out


def case_eob_only():
    """a stored block, then a dynamic block whose literal/length set is the end-of-block code alone, one bit: incomplete, and taken
    by zlib"""
    s = Stream().stored(b">eob_only\nACGTACGTAC\n").dynamic([], [0] * 256 + [1], [0], True)
    return [_m(s)]


def case_fixed(rng):
    """fixed blocks: 9-bit literals (bytes from 144 on) in a header line, length symbols 280 .. 285"""
    hdr = b">fixed " + bytes(range(144, 256)) + bytes([143, 144, 255, 200]) + b"\n"
    tokens = _lits(hdr + _seq(rng, 20))
    for s in range(280, 285):
        tokens += [(LEN_BASE[s - 257], 5), (LEN_BASE[s - 257] + 31 if s < 284 else 258, 7, s == 284)]
    tokens += [(258, 1), 10]
    s = Stream().fixed(tokens, True)
    assert all(any(k.startswith("len_%d_" % n) for k in s.census) for n in range(280, 286))
    return [_m(s)]


def case_blocks(rng):
    out = []
    s = Stream().stored(b">blocks\n")
    for i in range(299):                                    # 300 blocks, the three types in turn, padding bits of either kind
        piece = _seq(rng, 1 + i % 7)
        tokens = _lits(piece) + ([(3 + i % 9, 1 + i % 5)] if i % 4 == 0 else [])
        if i % 3 == 0:
            s.fixed(tokens)
        elif i % 3 == 1:
            _auto_dynamic(s, tokens, rng, last=False)
        else:
            s.stored(piece, ones=i % 2 == 1)
    s.fixed([10], True)
    assert len(s.blocks) == 301 and s.census["type0"] >= 100 and s.census["type1"] >= 100 and s.census["type2"] >= 99
    out.append(_m(s))
    # a stored block behind a Huffman block, every padding bit set; empty stored blocks, not final and final; an empty fixed final block
    s = Stream().fixed(_lits(b">padding\nAC"))
    assert s.w.n not in (0, 5, 6, 7)                        # (there are padding bits behind the three of the block's header)
    s.stored(b"GT\n", ones=True).stored(b"").stored(b"", True)
    out.append(_m(s))
    s = Stream().stored(b">empty_fixed\nACGT\n").fixed([])
    s.stored(b"", ones=True).fixed([], True)
    out.append(_m(s))
    return out


def case_expansion():
    """ISIZE 65 536 out of a few hundred bytes: 254 x (258, 1), the last match ending exactly at ISIZE"""
    s = Stream().fixed(_lits(b">x\nA") + [(258, 1)] * 254, True)
    assert len(s.text) == 65536 and len(s.w.buf) < 500
    return [_m(s), _m(Stream().stored(b"\n", True))]


def case_subfields(rng):
    out = []
    for name, kw in (("before", dict(before=[(b"XY", b"abc")])), ("after", dict(after=[(b"ZZ", b"")])),
                     ("both", dict(before=[(b"AB", b"\0" * 5), (b"CB", b"BC")], after=[(b"BD", b"BC\x02\x00")])),
                     ("wide", dict(before=[(b"Q%d" % i, bytes(rng.randrange(256) for _ in range(30 + i))) for i in range(9)]))):
        tokens = _lits(b">sub_" + name.encode() + b"\n" + _seq(rng, 30)) + [(9, 4), 10]
        out.append(_m(_auto_dynamic(Stream(), tokens, rng), **kw))
    assert len(out[-1][0]) > 300
    return out


def named_members(shift=0):
    """[(member, text)] of every named case, in one FASTA; `shift` more bytes in the first header line move every later member's
    text to another alignment"""
    rng = random.Random(11)
    first = _m(Stream().stored(b">craft" + b"x" * shift + b"\n", True))
    return ([first] + case_deep() + case_lengths(rng) + case_far(rng) + case_overlaps(rng) + case_headers(rng) + case_special_sets(rng) +
            case_eob_only() + case_fixed(rng) + case_blocks(rng) + case_subfields(rng) + case_expansion())


# ---- the seeded generator --------------------------------------------------------------------------------------------------------
_HEADER_BYTES = bytes(b for b in range(256) if b != 10)


def _random_text(rng, n, far):
    """FASTA-like text of n bytes: header lines of any bytes, sequence lines with runs and short periods; `far`: a stretch
    that comes again 32 507 .. 32 768 bytes on"""
    out = bytearray()
    while len(out) < n:
        out += b">" + bytes(rng.choices(_HEADER_BYTES, k=rng.randint(0, 40))) + b"\n"
        for _ in range(rng.randint(0, 12)):
            kind = rng.random()
            if kind < 0.15:
                line = bytes([rng.choice(SEQ)]) * rng.randint(1, 300)
            elif kind < 0.3:
                line = (_seq(rng, rng.randint(2, 8)) * 80)[:rng.randint(1, 300)]
            else:
                line = _seq(rng, rng.randint(0, 80))
            out += line + b"\n"
    out = out[:n - 1] + b"\n"
    if far:
        body = bytearray(b">far\n" + _seq(rng, n))
        at = 5
        while at + 32768 + 300 < len(body):
            d, k = rng.randint(FAR, 32768), rng.randint(20, 300)
            body[at + d:at + d + k] = body[at:at + k]
            at += rng.randint(300, 3000)
        out = body[:n - 1] + b"\n"
    return bytes(out)


def _random_tokens(rng, text):
    grams, tokens, p, n = {}, [], 0, len(text)
    while p < n:
        cands = grams.get(text[p:p + 3], ()) if p + 3 <= n else ()
        lo = bisect.bisect_left(cands, p - 32768)      # (positions in rising order: the window starts here)
        if lo < len(cands) and rng.random() < 0.7:
            q = cands[rng.choice((lo, len(cands) - 1, rng.randrange(lo, len(cands))))]
            k = 0
            while k < 258 and p + k < n and text[q + k] == text[p + k]:
                k += 1
            k = k if rng.random() < 0.6 else rng.randint(3, k)
            tokens.append((k, p - q, True) if k == 258 and rng.random() < 0.5 else (k, p - q))
        else:
            k = 1
            tokens.append(text[p])
        for i in range(p, p + k):
            grams.setdefault(text[i:i + 3], []).append(i)
        p += k
    return tokens


def legal_members(seed, n, big=0):
    """n random members of at most 4 KB of text (and `big` of 40 .. 64 KB in front): random token streams over FASTA-like text, cut
    into 1 .. 5 blocks of random type; the dynamic blocks have random complete sets of up to 15 bits and a random legal use of 16,
    17 and 18.  Every one is checked against zlib as it is made.  -> ([(member, text)], census)"""
    rng = random.Random(seed)
    out, census = [], collections.Counter()
    for i in range(big + n):
        text = _random_text(rng, rng.randint(40000, 65536) if i < big else rng.choice((200, 1000, 4096)) - rng.randrange(170), i < big)
        tokens = _random_tokens(rng, text)
        cuts = sorted(rng.sample(range(1, len(tokens)), min(rng.randint(0, 4), len(tokens) - 1)))
        s = Stream()
        for a, b in zip([0] + cuts, cuts + [len(tokens)]):
            part, last, kind = tokens[a:b], b == len(tokens), rng.randrange(4)
            weights = None
            if sum(1 if isinstance(t, int) else t[0] for t in part) > 6000:   # (a member has to fit BSIZE: no long part at a byte a base)
                kind = 2
                weights = collections.Counter(t if isinstance(t, int) else len_code(t[0], len(t) > 2 and t[2])[0] for t in part)
            if kind == 0:
                s.stored(apply(part, s.text), last, ones=rng.random() < 0.5)
            elif kind == 1:
                s.fixed(part, last)
            else:
                ls, ds = used_symbols(part)
                ls |= set(rng.sample(range(286), rng.choice((0, 0, 1, 5, 40))))
                if len(ls) == 1:
                    ls.add(10)
                if ds and (len(ds) > 1 or rng.random() < 0.5):
                    ds |= set(rng.sample(range(30), rng.choice((0, 1, 6))))
                deep = rng.choice((0.1, 0.5, 0.9))
                ll = set_from(ls, rng.randint(max(257, max(ls) + 1), 286), rng, 15, deep, weights)
                dl = set_from(ds, rng.randint(max(ds) + 1, 30), rng, 15, deep) if ds else [0] * rng.randint(1, 30)
                seq = cl_rle(ll + dl, rng)
                s.dynamic(part, ll, dl, last, cl_seq=seq, cl_lens=cl_code_lengths(seq, rng), hclen=rng.choice((None, None, 19)))
        assert bytes(s.text) == text
        out.append((good_member(s), text))
        census += s.census
        census["blocks3"] += len(s.blocks) >= 3
    return out, census


CENSUS_KEYS = ("bits15", "far", "overlap", "blocks3", "type0", "type1", "type2", "hclen_below_19", "single_distance_code")
GENERATOR_SEED, GENERATOR_N, GENERATOR_BIG = 20, 300, 5


# ---- malformed members ------------------------------------------------------------------------------------------------------------
OK, IN_END, OUT_FULL, BLOCK_TYPE, STORED_LEN, CODE_LENGTHS, SYMBOL, DISTANCE, SIZE, TRAILING, CRC, PLAN = range(12)   # BgzfStatus
REFUSED, STATUS, BAD_CRC = 0, 1, 2   # the outcome of a file: refused by the walk, a member's status, a member's CRC
PAD = [("B", 0, 8)] * 4              # input behind the wrong place: the decoder reads up to 15 bits before it calls bits no code


def _bad(stream, cut=None):
    return member(stream.bad(cut), b"", isize=max(1, len(stream.text)))


def malformed():
    """{name: (file bytes, outcome, BgzfStatus)}: one malformed member (and the end marker) per file"""
    text = b">bad\nACGTACGTAC\n"
    lit = _lits(text)
    ll_ok = fit_lengths(257, {}, used_symbols(lit)[0], SPARE)
    out = {}

    def add(name, m, outcome, status):
        out[name] = (m + _bgzf.EOF_MARKER, outcome, status)

    def dyn(name, ll, dl, tokens=lit, status=CODE_LENGTHS, **kw):
        add(name, _bad(Stream().dynamic(tokens + PAD, ll, dl, True, strict=False, **kw)), STATUS, status)

    # code sets and header counts
    three = [0] * 257
    three[65] = three[67] = three[256] = 1
    dyn("oversubscribed_literals", three, [0], tokens=[65, 67], eob=True)
    dyn("oversubscribed_distances", ll_ok, [1, 1, 1])
    dyn("oversubscribed_code_lengths", ll_ok, [0], cl_lens=[1 if i in (0, 4, 5) else 3 if i in (3, 6) else 0 for i in range(19)],
        cl_seq=[l if l in (0, 3, 4, 5, 6) else 0 for l in ll_ok] + [0])
    two = [0] * 257
    two[65] = two[256] = 2
    dyn("incomplete_literals_two_codes_of_two_bits", two, [0], tokens=[65, 65])
    dyn("incomplete_distances_two_codes_of_two_bits", ll_ok, [2, 2])
    # (one code of one bit is the only incomplete set zlib takes: a second code beside it, or one code of another length, is none)
    one_two = [0] * 257
    one_two[256], one_two[65] = 1, 2
    dyn("incomplete_literals_two_codes_of_one_and_two_bits", one_two, [0], tokens=[65, 65])
    dyn("incomplete_distances_two_codes_of_one_and_two_bits", ll_ok, [1, 2])
    dyn("incomplete_literals_one_code_of_two_bits", [0] * 256 + [2], [0], tokens=[])
    dyn("incomplete_distances_one_code_of_two_bits", ll_ok, [2])
    cl = [0] * 19
    cl[0] = cl[8] = 2
    dyn("incomplete_code_lengths", [0] + [8] * 256, [0], cl_lens=cl, cl_seq=[0] + [8] * 256 + [0])
    no_eob = list(ll_ok)
    no_eob[256], no_eob[SPARE[-1]] = 0, ll_ok[256]
    assert kraft(no_eob) == 32768
    dyn("no_end_of_block_code", no_eob, [0], eob=False)
    all8 = dict(cl_lens=[1 if i == 8 else 2 if i in (0, 16) else 0 for i in range(19)])
    dyn("16_at_index_0", [8] * 257, [0], cl_seq=[(16, 3)] + [8] * 254 + [0], tokens=[], eob=False, **all8)
    # a repeat past nlen + ndist and nothing else wrong: only zeros spill, so that without the decoder's check of the repeat both sets
    # are legal and the member inflates; and a long one from index 257 of 316, which without the check writes lengths 316 .. 394,
    # past the 320 the table has room for
    dyn("repeat_past_the_total", ll_ok, [0], cl_seq=cl_rle(ll_ok) + [(17, 3)])
    dyn("long_repeat_past_the_total", ll_ok + [0] * 29, [0] * 30, cl_seq=cl_rle(ll_ok) + [(18, 138)])
    dyn("hclen_4_says_no_length_but_0", [0] * 257, [0], cl_seq=[(18, 138), (18, 120)], cl_lens=[1 if i in (0, 18) else 0 for i in range(19)],
        hclen=4, tokens=[], eob=False)
    for n in (287, 288):
        dyn("hlit_%d" % n, ll_ok + [0] * (n - 257), [0])
    for n in (31, 32):
        dyn("hdist_%d" % n, ll_ok, [0] * n)
    # symbols
    for s in (286, 287):
        add("fixed_literal_symbol_%d" % s, _bad(Stream().fixed(lit + [("L", s)] + PAD, True)), STATUS, SYMBOL)
    for s in (30, 31):
        add("fixed_distance_symbol_%d" % s, _bad(Stream().fixed(lit + [("L", 257), ("D", s)] + PAD, True)), STATUS, SYMBOL)
    ll_m = fit_lengths(258, {}, used_symbols(lit + [(3, 1)])[0], SPARE)
    dyn("unused_bit_of_the_single_distance_code", ll_m, [1], tokens=lit + [("L", 257), ("B", 1, 1)], status=SYMBOL)
    dyn("length_symbol_without_a_distance_code", ll_m, [0], tokens=lit + [("L", 257)], status=SYMBOL)
    add("unused_bit_of_the_end_of_block_only_set",
        _bad(Stream().stored(text).dynamic([("B", 1, 1)] + PAD, [0] * 256 + [1], [0], True, strict=False)), STATUS, SYMBOL)
    # structure
    add("distance_is_out_plus_1", _bad(Stream().fixed(lit + [(3, len(lit) + 1)] + PAD, True)), STATUS, DISTANCE)
    s = Stream().fixed(lit)
    s.w.bits(1, 1)
    s.w.bits(3, 2)
    s.w.bits(0, 32)
    add("block_type_3", _bad(s), STATUS, BLOCK_TYPE)
    add("nlen_mismatch", _bad(Stream().stored(text, True, nlen=(len(text) ^ 0xFFFF) ^ 0x100)), STATUS, STORED_LEN)
    add("stored_len_beyond_the_input", _bad(Stream().stored(text, True, length=len(text) + 1)), STATUS, IN_END)
    # sizes: the deflate data is legal, the member around it is not
    for name, s in (("literal", Stream().fixed(lit + [65], True)), ("match", Stream().fixed(lit + [(3, 4)], True)),
                    ("stored_block", Stream().fixed(lit).stored(b"A", True))):
        t = bytes(s.text)
        add("one_byte_more_than_isize_by_a_" + name, bad_member(s.legal(), t, isize=len(t) - 1), STATUS, OUT_FULL)
    s = Stream().fixed(lit, True)
    add("one_byte_less_than_isize", bad_member(s.legal(), text, isize=len(text) + 1), STATUS, SIZE)
    add("trailing_byte_behind_the_final_block", bad_member(s.legal() + b"\0", text), STATUS, TRAILING)
    # the input ends inside a code, inside length extra bits, inside distance extra bits
    deep = [0] * 257
    for i, sym in enumerate([65, 67, 71, 84, 10, 256, 62, 98, 97, 100] + SPARE[:6]):
        deep[sym] = min(i + 1, 15)
    s = Stream().dynamic(lit, deep, [0], False, strict=True)
    at = s.w.pos()
    s.tokens([SPARE[5]], canonical(deep), {})
    assert canonical(deep)[SPARE[5]][1] == 15 and at // 8 + 1 < (at + 15 + 7) // 8
    add("input_ends_inside_a_code", _bad(s, cut=at // 8 + 1), STATUS, IN_END)
    for k in range(8):
        s = Stream().fixed(lit + [200] * k, False)       # (9-bit literals move the place by one bit each)
        s._head(True, 1)
        s.w.code(*canonical(FIXED_LL)[284])
        at = s.w.pos()                                    # five extra bits from here
        if 4 <= at % 8:
            break
    s.w.bits(31, 5)
    s.w.bits(0, 16)
    add("input_ends_inside_length_extra_bits", _bad(s, cut=at // 8 + 1), STATUS, IN_END)
    s = Stream().fixed(lit, False)
    s._head(True, 1)
    s.w.code(*canonical(FIXED_LL)[257])
    s.w.code(29, 5)
    at = s.w.pos()                                        # thirteen extra bits from here
    s.w.bits(0, 13)
    s.w.bits(0, 16)
    add("input_ends_inside_distance_extra_bits", _bad(s, cut=at // 8 + 1), STATUS, IN_END)
    # at the walk
    good = Stream().fixed(lit, True)
    raw = good.legal()
    add("two_bc_subfields", member(raw, text, subfields=[(b"BC", None), (b"BC", None)]), REFUSED, OK)
    add("bc_with_slen_3", member(raw, text, subfields=[(b"BC", 1)]), REFUSED, OK)
    for n in (1, 2, 3):
        add("stray_bytes_in_the_extra_field_%d" % n, member(raw, text, stray=b"\0" * n), REFUSED, OK)
    add("isize_65537", bad_member(raw, text, isize=65537), REFUSED, OK)
    return out
