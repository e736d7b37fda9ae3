"""The contract of mxg_compose_pieces (include/ntjoin_mx.h, row f11) restated in Python, from its text: a linear walk over the pieces
of every inner record, no prefix table and no bisection.  What mxg_compose_pieces and tools/compose_check.cpp must reproduce.

A table is a list of records; a record is a list of pieces (record, start, end, kind)."""
FWD, REV, GAP = 0, 1, 2
EINVAL, ELIMIT = -1, -5
MAX_LEN = 2 ** 32 - 1
COMP = str.maketrans("ACGTUNMRWSYKVHDBacgtunmrwsykvhdb", "TGCAANKYWSRMBDHVtgcaankywsrmbdhv")   # bin/ntjoin_utils.py:145-150


class Refused(ValueError):
    def __init__(self, code, why):
        super().__init__(why)
        self.code = code


def record_length(rec):
    return sum(e - s for _, s, e, _ in rec)


def check_table(table, ref_len=None):
    """a valid table (every record has a piece, every piece start < end and a known kind, no record beyond 2^32 - 1 bases) whose
    sequence pieces lie inside the records they name, when their lengths are given"""
    for rec in table:
        if not rec:
            raise Refused(EINVAL, "a record without pieces")
        for r, s, e, kind in rec:
            if kind not in (FWD, REV, GAP) or s >= e:
                raise Refused(EINVAL, "an unknown kind or an empty piece")
            if kind != GAP and ref_len is not None and (r >= len(ref_len) or e > ref_len[r]):
                raise Refused(EINVAL, "a piece outside the record it names")
        if record_length(rec) > MAX_LEN:
            raise Refused(ELIMIT, "a record longer than 2^32 - 1 bases")


def expand(piece, inner):
    "what one outer piece becomes"
    r, a, b, kind = piece
    if kind == GAP:
        return [(0, 0, b - a, GAP)]
    out, at = [], 0
    for qr, qs, qe, qk in inner[r]:
        n = qe - qs
        lo, hi = max(a, at) - at, min(b, at + n) - at   # the part of the inner piece's own spelling inside [a, b)
        at += n
        if lo >= hi:
            continue
        if qk == GAP:
            out.append((0, 0, hi - lo, GAP))
        elif qk == FWD:
            out.append((qr, qs + lo, qs + hi, FWD))
        else:   # spelled from its end downwards
            out.append((qr, qe - hi, qe - lo, REV))
    if kind == REV:
        out = [(qr, qs, qe, qk if qk == GAP else FWD + REV - qk) for qr, qs, qe, qk in reversed(out)]
    return out


def compose(outer, inner):
    check_table(inner)
    check_table(outer, [record_length(rec) for rec in inner])
    result = []
    for rec in outer:
        res = []
        for piece in rec:
            for o in expand(piece, inner):
                if o[3] == GAP and res and res[-1][3] == GAP:
                    res[-1] = (0, 0, res[-1][2] + o[2], GAP)
                else:
                    res.append(o)
        result.append(res)
    return result


def spell(rec, seqs):
    "the sequence a record's pieces spell over the strings `seqs`"
    parts = []
    for r, s, e, kind in rec:
        if kind == GAP:
            parts.append("N" * (e - s))
        else:
            assert e <= len(seqs[r])
            t = seqs[r][s:e]
            parts.append(t if kind == FWD else t[::-1].translate(COMP))
    return "".join(parts)
