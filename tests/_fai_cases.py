"""FASTA texts for the .fai tests (tests/test_fai_cpu.py: the host program over fai_scan.h; tests/test_gpu_fai.py: mxg_write_fai):
the shapes the device route has a path of its own for, and one file per rule of refusal.  The work items are cut at multiples of 4096
bytes of the file, so a record of a little over 12 288 bytes of text lies in three or four of them.

    shapes()   -> {name: text}            accepted files
    refusals() -> {name: (text, "bad")}   refused files and the id of the record that is refused
"""
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
