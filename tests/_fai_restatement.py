"""What mxg_write_fai writes, restated in plain Python from the rules of its contract (include/ntjoin_mx.h), not from the code of the
device route: the .fai of a FASTA text as `samtools faidx` makes it, the refusals, and faidx's way back from a row to the bases.

    records(text)      -> [(name, text_off, se)]: header lines are '>' at the start of a line, the name ends at the first blank
    index(text)        -> ([(name, length, offset, linebases, linewidth)], dropped names); raises Refused(record index, name, offset)
    fai_bytes(text)    -> the file
    fetch(row, text, lo, hi) -> bases [lo, hi) of the row's record by OFFSET + lo / LINEBASES * LINEWIDTH + lo % LINEBASES
    gzi_bytes(members) -> the .gzi of members [(compressed offset, text offset)] that hold text
"""
import struct


class Refused(Exception):
    def __init__(self, record, name, offset):
        super().__init__("record %d (%s): line at byte %d" % (record, name, offset))
        self.record, self.name, self.offset = record, name, offset


def records(text):
    heads = []
    p = 0
    while p < len(text):
        if text[p:p + 1] == b">" and (p == 0 or text[p - 1:p] == b"\n"):
            end = text.find(b"\n", p)
            end = len(text) if end < 0 else end
            heads.append((p, end))
            p = end + 1
        else:
            nxt = text.find(b"\n>", p)
            p = len(text) if nxt < 0 else nxt + 1
    out = []
    for r, (at, end) in enumerate(heads):
        line = text[at + 1:end]
        stop = len(line)
        for i, c in enumerate(line):
            if c in b" \t\r\n":
                stop = i
                break
        out.append((line[:stop].decode("latin-1"), min(end + 1, len(text)), heads[r + 1][0] if r + 1 < len(heads) else len(text)))
    return out


def _is_base(c):
    return 0x21 <= c <= 0x7E


def _lines(T):
    "T split at \\n -> [(start in T, bytes with the line end)]"
    out, p = [], 0
    while p < len(T):
        q = T.find(b"\n", p)
        q = len(T) if q < 0 else q + 1
        out.append((p, T[p:q]))
        p = q
    return out


def _end_of(line):
    return b"\r\n" if line.endswith(b"\r\n") else b"\n" if line.endswith(b"\n") else b""


def row_of(T, name, text_off, r, last_record):
    if not T:
        return (name, 0, text_off, 0, 0)
    lines = _lines(T)
    first = lines[0][1]
    width, bases = len(first), sum(1 for c in first if _is_base(c))
    body = [ln[:len(ln) - len(_end_of(ln))] for _, ln in lines]
    nonempty = [i for i, b in enumerate(body) if b]
    last = nonempty[-1] if nonempty else -1
    for i, (at, ln) in enumerate(lines):
        ok = all(_is_base(c) for c in body[i])  # (a \r is legal directly in front of the \n only: it is part of the line end then)
        if i < last:
            ok = ok and len(ln) == width and len(body[i]) == bases
        elif i == last:
            ok = ok and 1 <= len(body[i]) <= bases and (_end_of(ln) == _end_of(first) or _end_of(ln) == b"")
        else:
            ok = ok and last_record  # empty lines follow only behind the last record of the file
        if not ok:
            raise Refused(r, name, text_off + at)
    return (name, sum(1 for c in T if _is_base(c)), text_off, bases, width)


def index(text):
    recs = records(text)
    rows, seen, dropped = [], set(), []
    for r, (name, lo, se) in enumerate(recs):
        row = row_of(text[lo:se], name, lo, r, r + 1 == len(recs))
        if name in seen:
            dropped.append(name)
            continue
        seen.add(name)
        rows.append(row)
    return rows, dropped


def format_rows(rows):
    return "".join("%s\t%d\t%d\t%d\t%d\n" % row for row in rows).encode("latin-1")


def fai_bytes(text):
    return format_rows(index(text)[0])


def parse(fai):
    rows = []
    for line in fai.decode("latin-1").splitlines():
        f = line.split("\t")
        rows.append((f[0], int(f[1]), int(f[2]), int(f[3]), int(f[4])))
    return rows


def fetch(row, text, lo, hi):
    _, _, offset, linebases, linewidth = row
    return bytes(text[offset + i // linebases * linewidth + i % linebases] for i in range(lo, hi))


def bases_of(text, lo, se):
    return bytes(c for c in text[lo:se] if _is_base(c))


def gzi_bytes(members):
    "members: (compressed offset, text offset) of every member that holds text, in file order"
    rest = members[1:]
    return struct.pack("<Q", len(rest)) + b"".join(struct.pack("<QQ", c, u) for c, u in rest)


def parse_gzi(b):
    (n,) = struct.unpack_from("<Q", b, 0)
    assert len(b) == 8 + 16 * n
    return [struct.unpack_from("<QQ", b, 8 + 16 * i) for i in range(n)]
