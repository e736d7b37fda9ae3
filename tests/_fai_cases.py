"""FASTA texts for the .fai tests (tests/test_fai_cpu.py: the host program over fai_scan.h; tests/test_gpu_fai.py: mxg_write_fai):
the shapes the device route has a path of its own for, and one file per rule of refusal.  The work items are cut at multiples of 4096
bytes of the file, so a record of a little over 12 288 bytes of text lies in three or four of them.

    shapes()   -> {name: text}            accepted files
    refusals() -> {name: (text, "bad")}   refused files and the id of the record that is refused
    carry_text(at, span, ...) -> text     `at` work items of tiny records, then the record "long" over `span` items (CARRIES: the
                                          places where the scan over the items carries from tile to tile and from round to round)
    items_of(text) -> [items per record]  the cutting rule restated
    tiny_records(n, dup) -> text          n records of a few bases under names of growing length (the offset scan's borders)
"""
import functools
import random

TILE = 4096
WIDTHS = (1, 15, 16, 17, 60, 255, 256, 4095, 4096, 4097)
SPAN = 3 * TILE + 1  # bases of a record that reaches into a fourth item whatever its line width


def seq(rng, n):
    return "".join(rng.choice("ACGTACGTACGTacgtNn") for _ in range(n))


def fold(s, width, eol="\n", end=True):
    "s in lines of `width` bases; end=False: the last line has no line end"
    lines = [s[p:p + width] for p in range(0, len(s), width)]
    return eol.join(lines) + (eol if end and lines else "")


def header(name, desc="", eol="\n"):
    return ">" + name + desc + eol


def padded_header(at, name, mod, eol="\n"):
    "a header line at offset `at` of the file whose sequence text starts at an offset = mod (modulo 4096)"
    base = len(">" + name + " " + eol)
    return ">" + name + " " + "p" * ((mod - at - base) % TILE) + eol


def _width_records(rng, eol):
    "(name, bases, width) for every width: a short last line, a last line of one base, a full last line"
    out = []
    for w in WIDTHS:
        full = (SPAN + w - 1) // w * w
        if w > 2:
            out.append(("w%d_short" % w, full + max(1, w // 2), w))
        if w > 1:
            out.append(("w%d_one" % w, full + 1, w))
        out.append(("w%d_full" % w, full, w))
    return [(name, seq(rng, n), w) for name, n, w in out]


def shapes():
    rng = random.Random(20)
    out = {}
    for tag, eol in (("lf", "\n"), ("crlf", "\r\n")):
        recs = _width_records(rng, eol)
        body = "".join(header(name, eol=eol) + fold(s, w, eol) for name, s, w in recs)
        # the end of the file: a full last line with and without its line end, a short one and a single base without
        for end_tag, n_last, end in (("full", 120, True), ("full_noeol", 120, False), ("short_noeol", 97, False), ("one_noeol", 61, False)):
            out["widths_%s_%s" % (tag, end_tag)] = body + header("last", eol=eol) + fold(seq(rng, SPAN // 60 * 60 + n_last), 60, eol, end)
        # single-line records
        out["single_" + tag] = "".join(header("s%d" % n, eol=eol) + seq(rng, n) + eol for n in (1, 4095, 4096, 12289))
        out["single_%s_noeol" % tag] = header("a", eol=eol) + seq(rng, 12289) + eol + header("b", eol=eol) + seq(rng, 4097)
        # a '\r' (or, for "\n", the last base) at offset 4095 of a tile and its '\n' in the next
        t = padded_header(0, "split", 0, eol)
        out["split_" + tag] = t + fold(seq(rng, 3 * (TILE - len(eol) + 1) + 5), TILE - len(eol) + 1, eol) + header("after", eol=eol) + fold(seq(rng, 100), 60, eol)
        # the sequence text at offsets 0, 1 and 4095 of a tile
        t = ""
        for mod in (0, 1, 4095):
            t += padded_header(len(t), "m%d" % mod, mod, eol) + fold(seq(rng, SPAN + 77), 60, eol)
            t += padded_header(len(t), "m%d_line" % mod, mod, eol) + seq(rng, SPAN) + eol
        out["offsets_" + tag] = t
        # records without text, between others and last; empty lines behind the last record
        out["zero_" + tag] = (header("z0", eol=eol) + header("a", " first", eol) + fold(seq(rng, 130), 60, eol) + header("z1", eol=eol) +
                              header("z2", "\tx", eol) + header("b", eol=eol) + fold(seq(rng, 9000), 70, eol) + header("z3", eol=eol))
        out["zero_%s_noeol" % tag] = header("a", eol=eol) + fold(seq(rng, 130), 60, eol) + ">z"
        out["trailing_" + tag] = header("a", eol=eol) + fold(seq(rng, 130), 60, eol) + header("b", eol=eol) + fold(seq(rng, SPAN), 60, eol) + eol * 3
        out["only_empty_" + tag] = header("a", eol=eol) + fold(seq(rng, 10), 60, eol) + header("b", eol=eol) + eol * 2
    # headers with descriptions and tabs
    out["headers"] = (header("id1", " a description > with a bracket") + fold(seq(rng, 200), 60) + header("id2", "\tcol\tcol") + fold(seq(rng, 61), 60) +
                      header("id|3.1", "  two blanks") + fold(seq(rng, 60), 60) + header("", " no name") + fold(seq(rng, 5), 60))
    # printable characters that are no nucleotides count as bases
    out["printable"] = header("p") + fold("".join(chr(0x21 + i % 94) for i in range(500)).replace(">", "X"), 50)
    return {k: v.encode("latin-1") for k, v in out.items()}


def duplicates():
    rng = random.Random(21)
    t = ""
    for name in ("a", "b", "a", "c", "b", "a"):
        t += header(name) + fold(seq(rng, rng.randint(50, 300)), 60)
    return t.encode("latin-1")


def _lines(rng, n, width=60):
    return [seq(rng, width) for _ in range(n)]


def refusals():
    "every rule once with the offence in the record's first item (line 2) and once in its third (line 150 of 230: byte 9150)"
    rng = random.Random(22)
    out = {}

    def wrap(lines, behind="", eol="\n", following=True):
        t = header("good0") + fold(seq(rng, 500), 60) + header("bad", " the refused one") + "".join(x + eol for x in lines) + behind
        if following:
            t += header("good1") + fold(seq(rng, 5000), 80)
        return t

    for where, n, at in (("first", 230, 2), ("third", 230, 150)):
        base = _lines(rng, n)
        def with_line(new, insert=False):
            ls = list(base)
            if insert:
                ls.insert(at, new)
            else:
                ls[at] = new
            return ls
        out["longer_middle_" + where] = wrap(with_line(seq(rng, 61)))
        out["shorter_middle_" + where] = wrap(with_line(seq(rng, 59)))
        out["empty_middle_" + where] = wrap(with_line("", insert=True))
        out["space_" + where] = wrap(with_line(base[at][:20] + " " + base[at][21:]))
        out["tab_" + where] = wrap(with_line(base[at][:20] + "\t" + base[at][21:]))
        out["lone_cr_" + where] = wrap(with_line(base[at][:20] + "\r" + base[at][21:]))
        out["nul_" + where] = wrap(with_line(base[at][:20] + "\0" + base[at][21:]))
    # at the record's end: in its first item (a record of two lines) and beyond its third
    for where, n in (("first", 2), ("third", 230)):
        base = _lines(rng, n)
        out["empty_behind_not_last_" + where] = wrap(base, behind="\n")
        out["last_longer_" + where] = wrap(base[:-1] + [seq(rng, 61)])
        out["last_other_end_" + where] = wrap(base[:-1], behind=seq(rng, 30) + "\r\n")
        out["last_longer_end_of_file_" + where] = wrap(base[:-1], behind=seq(rng, 61), following=False)
    return {k: (v.encode("latin-1"), "bad") for k, v in out.items()}


# ---- the carries of the scan over the work items (k_fai_tile_agg -> k_fai_tile_scan -> k_fai_rows) ----
ITEMS_TILE = 256             # items a tile
ITEMS_ROUND = 256 * 256      # items a round of k_fai_tile_scan: 256 tiles


def _n_items(lo, se):
    "text [lo, se) of one record cut at the aligned 4096-byte borders of the file"
    return 0 if se <= lo else (se - 1) // TILE - lo // TILE + 1


def items_of(text):
    """work items per record: a record's text, from the byte behind its header line to the next header line (or the end of the
    file), is cut at the multiples of 4096 bytes of the file; a record without text has none (the rule tools/fai_check.cpp states)"""
    from tests import _fai_restatement as R
    return [_n_items(lo, se) for _, lo, se in R.records(text)]


def carry_text(at, span, tail=5, bad=(), seed=23):
    """exactly `at` work items of tiny records with unique names (one in eleven without text, two in eleven with CRLF, text that
    straddles a border of the file's tiles where it falls: two items), the last of them three full lines of 7 bases; then the record
    "long" in lines of 60 bases + LF over exactly `span` items, ending with a short line 2000 bytes into its last item; then `tail`
    small records and two without text.  bad: items of "long" (counted from 0) in which one whole line has 59 bases"""
    assert at >= 1 and span >= 2
    rng = random.Random(seed)
    stock = seq(rng, 4099)
    parts, pos, n, i = [], 0, 0, 0

    def put(s):
        nonlocal pos
        parts.append(s)
        pos += len(s)

    while n < at:
        kind = i % 11
        eol = "\r\n" if kind in (3, 7) else "\n"
        head = header("f%d" % i, eol=eol)
        i += 1
        front = n == at - 1  # (the record in front of "long": another width, no short last line)
        if front:
            body = fold(stock[i % 4000:i % 4000 + 21], 7)
        elif kind == 5:
            body = ""
        else:
            body = stock[i % 4000:i % 4000 + 3 + i % 9] + eol
        k = _n_items(pos + len(head), pos + len(head) + len(body))
        if n + k > (at if front else at - 1):  # (it would take the place of "long" or of the record in front: no text, try again)
            body, k = "", 0
        put(head + body)
        n += k
    head = header("long", " over %d items" % span)
    lo = pos + len(head)
    q, r = divmod((lo // TILE + span - 1) * TILE + 2000 - lo - 1, 61)
    lines = [(stock * 2)[(7 * j) % 4000:(7 * j) % 4000 + 60] for j in range(q)] + [stock[:r or 30]]
    for j in bad:
        at_line = ((lo // TILE + j) * TILE - lo) // 61 + 2  # (a line that lies inside item j)
        lines[at_line] = lines[at_line][:59]
    put(head + "\n".join(lines) + "\n")
    for j in range(tail):
        put(header("t%d" % j, " tail") + fold(stock[j:j + 100 + j], 70))
    put(">x\n>y\n")
    return "".join(parts).encode("latin-1")


_R = ITEMS_ROUND
# name -> (arguments of carry_text, refused?); "long" begins on item `at`
CARRIES = {
    "tile": (dict(at=255, span=2), False),
    "last_of_round": (dict(at=_R - 1, span=2), False),
    "first_of_round": (dict(at=_R, span=2), False),
    "across": (dict(at=_R - 300, span=600), False),
    "second_round": (dict(at=2 * _R - 300, span=600), False),
    "exact_round": (dict(at=_R - 2, span=2, tail=0), False),
    "exact_round_plus_one": (dict(at=_R - 1, span=2, tail=0), False),
    "refusal_behind": (dict(at=_R - 300, span=600, bad=(400,)), True),
    "refusal_in_front": (dict(at=_R - 300, span=600, bad=(100, 400)), True),
}


@functools.lru_cache(maxsize=None)
def carry_case(name):
    return carry_text(**CARRIES[name][0])


# ---- the borders of the 64-bit scan over the rows' line sizes (1 024 offsets a tile, 262 144 a round) ----
@functools.lru_cache(maxsize=None)
def tiny_records(n, dup=()):
    """n records of 1 .. 4 bases on one line; the names grow (r0, r1, ..., with a run of 'x' that gets longer every 37 records), so
    the lines of the index differ in size; record i in `dup` bears the name of record i - 1 (it gets no line)"""
    parts = []
    for i in range(n):
        j = i - 1 if i in dup else i
        parts.append(">r%d%s\n%s\n" % (j, "x" * (j // 37 % 23), "ACGT"[:1 + i % 4]))
    return "".join(parts).encode("latin-1")
