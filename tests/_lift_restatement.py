"""The contract of mxg_lift_prepare / mxg_lift_intervals / mxg_lift_bed (include/ntjoin_mx.h, row f15) restated in Python, from its
text: per feature a linear scan over ALL pieces of the table, no index, no sort and no bisection.  What the device route and
tools/lift_check.cpp must reproduce.

A table is a list of records; a record is a list of pieces (record, start, end, kind).  A feature is (record, start, end); a part is
(s_record, s_start, s_end, src_start, reverse)."""
import re

from tests import _compose_restatement as C

FWD, REV, GAP = C.FWD, C.REV, C.GAP
WHOLE, SPLIT, PARTIAL, LOST, INVALID, UNKNOWN = 0, 1, 2, 3, 4, 5
REASON = {SPLIT: "Split in new", PARTIAL: "Partially deleted in new", LOST: "Deleted in new", INVALID: "Invalid", UNKNOWN: "Unknown record"}
EINVAL, ELIMIT = C.EINVAL, C.ELIMIT
MAX_PARTS = 2 ** 31 - 1   # 2^31 parts or more are refused
Refused = C.Refused


def check(table, source_length):
    "what mxg_lift_prepare refuses"
    C.check_table(table, list(source_length))
    if len(source_length) >= 2 ** 31 - 1:
        raise Refused(ELIMIT, "too many source records")


def lift_one(table, source_length, feature):
    "-> (status, parts)"
    r, a, b = feature
    if r >= len(source_length) or a >= b or b > source_length[r]:
        return INVALID, []
    found = []
    index = 0
    for R, rec in enumerate(table):
        off = 0
        for pr, ps, pe, kind in rec:
            if kind != GAP and pr == r and ps < b and pe > a:
                lo, hi = max(a, ps), min(b, pe)
                if kind == FWD:
                    part = (R, off + lo - ps, off + hi - ps, lo, 0)
                else:
                    part = (R, off + pe - hi, off + pe - lo, lo, 1)
                found.append(((ps, index), part, hi - lo))
            off += pe - ps
            index += 1
    found.sort(key=lambda x: x[0])
    parts = [part for _, part, _ in found]
    lifted = sum(n for _, _, n in found)
    if not parts:
        return LOST, []
    if len(parts) == 1 and lifted == b - a:
        return WHOLE, parts
    if lifted < b - a:
        return PARTIAL, parts
    return SPLIT, parts


def lift(table, source_length, features, whole_only=False):
    "-> (statuses, part_first, parts); Refused as the entry points refuse"
    check(table, source_length)
    statuses, part_first, parts = [], [0], []
    for f in features:
        s, p = lift_one(table, source_length, f)
        statuses.append(s)
        if not (whole_only and s != WHOLE):
            parts.extend(p)
        part_first.append(len(parts))
    if len(parts) > MAX_PARTS - 1:
        raise Refused(ELIMIT, "2^31 parts or more")
    return statuses, part_first, parts


# ---- BED ---------------------------------------------------------------------------------------------------------------------------
_NUMBER = re.compile(rb"[0-9]{1,10}\Z")


def bed_lines(data):
    "the lines of a file (bytes), without their line ends"
    if not data:
        return []
    lines = data.split(b"\n")
    if lines[-1] == b"":   # the last line had its '\n'
        lines.pop()
    return [ln[:-1] if ln.endswith(b"\r") else ln for ln in lines]


def bed_feature(line, source_names):
    """-> (feature or None, forced status or None, rest or None, strand index in rest or None); a line that holds a feature"""
    f = line.split(b"\t")
    rest = b"\t".join(f[3:]) if len(f) >= 4 else None
    strand = None
    if len(f) >= 6 and f[5] in (b"+", b"-"):
        strand = len(b"\t".join(f[3:5])) + 1
    if len(f) < 3 or not _NUMBER.match(f[1]) or not _NUMBER.match(f[2]) or int(f[1]) > 2 ** 32 - 1 or int(f[2]) > 2 ** 32 - 1:
        return None, INVALID, rest, strand
    a, b = int(f[1]), int(f[2])
    if f[0] in source_names:
        return (source_names.index(f[0]), a, b), None, rest, strand   # (index: the first record of that name)
    return None, (INVALID if a >= b else UNKNOWN), rest, strand


def lift_bed(table, source_length, source_names, scaffold_names, data, whole_only=False):
    """-> (lifted bytes, unlifted bytes, stats dict).  Names are bytes."""
    check(table, source_length)
    source_names = list(source_names)
    lifted, unlifted = [], []
    stats = dict(lines=0, skipped=0, features=0, whole=0, split=0, partial=0, lost=0, invalid=0, unknown=0, parts=0)
    names = ("whole", "split", "partial", "lost", "invalid", "unknown")
    for line in bed_lines(data):
        stats["lines"] += 1
        if line == b"" or line.startswith((b"#", b"track", b"browser")):
            stats["skipped"] += 1
            continue
        stats["features"] += 1
        feature, status, rest, strand = bed_feature(line, source_names)
        parts = []
        if feature is not None:
            status, parts = lift_one(table, source_length, feature)
        stats[names[status]] += 1
        if status != WHOLE:
            unlifted.append(b"#" + REASON[status].encode() + b"\n" + line + b"\n")
            if whole_only:
                parts = []
        for R, s, e, _, rev in parts:
            out = scaffold_names[R] + b"\t%d\t%d" % (s, e)
            if rest is not None:
                tail = rest
                if rev and strand is not None:
                    tail = rest[:strand] + (b"-" if rest[strand:strand + 1] == b"+" else b"+") + rest[strand + 1:]
                out += b"\t" + tail
            lifted.append(out + b"\n")
            stats["parts"] += 1
    lifted, unlifted = b"".join(lifted), b"".join(unlifted)
    stats["lifted_bytes"], stats["unlifted_bytes"] = len(lifted), len(unlifted)
    return lifted, unlifted, stats
