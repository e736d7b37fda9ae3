"""Stand-in for the one pybedtools call chain ntJoin's tally_intersecting_segments makes (pybedtools and the bedtools binary are
not installed in the build container):

    BedTool(text, from_string=True).sort().intersect(b=<the same>, c=True, wa=True)

Contract: sort() orders the lines by chromosome, then start, then end (bedtools' own sort leaves the order of equal starts
undefined: ascending end is this project's rule, see tests/golden/adjust/README.md); intersect(c=True, wa=True) yields every line of
a, in a's order, with the number of lines of b on the same chromosome that share at least one base with it, half-open:
max(starts) < min(ends).  Intervals are taken to hold at least one base.  tests/test_adjust_cpu.py checks the counts against a
brute-force count.

EQUAL_START_LARGER_END_FIRST (off by default) makes sort() put the larger end first among equal starts: the generator of the
adjustment goldens runs every case under both orders and records whether the answer depends on the order."""
import bisect
import collections

Interval = collections.namedtuple("Interval", "chrom start end count")
EQUAL_START_LARGER_END_FIRST = False


class BedTool:
    def __init__(self, text, from_string=False):
        if not from_string:
            raise NotImplementedError("the stand-in reads BED text only")
        self.rows = []
        for line in (text if isinstance(text, list) else str(text).split("\n")):
            if isinstance(line, tuple):
                self.rows.append(line)
            elif line.strip():
                chrom, start, end = line.split("\t")[:3]
                self.rows.append((chrom, int(start), int(end)))

    def sort(self):
        if EQUAL_START_LARGER_END_FIRST:
            return BedTool(sorted(self.rows, key=lambda row: (row[0], row[1], -row[2])), from_string=True)
        return BedTool(sorted(self.rows), from_string=True)

    def intersect(self, b, c=False, wa=False):
        if not (c and wa):
            raise NotImplementedError("the stand-in counts only (c=True, wa=True)")
        starts, ends = collections.defaultdict(list), collections.defaultdict(list)
        for chrom, start, end in b.rows:
            starts[chrom].append(start)
            ends[chrom].append(end)
        for table in (starts, ends):
            for values in table.values():
                values.sort()
        # b ends at or before a's start, or begins at or after a's end: the two kinds exclude one another for intervals that hold a base
        return [Interval(chrom, start, end, bisect.bisect_left(starts[chrom], end) - bisect.bisect_right(ends[chrom], start))
                for chrom, start, end in self.rows]

    def __iter__(self):
        return iter(self.rows)
