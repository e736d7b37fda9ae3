"""Plain-Python restatement of the path adjustment stage: what ntJoin does to the paths between format_path and the
trimming / printing of the scaffolds, in seven phases.  Written from the stage's semantics; the goldens under tests/golden/adjust
(recorded from ntJoin's own functions) pin it.  Test infrastructure only.

A row is [contig, ori, start, end, contig_size, first_mx, terminal_mx, gap_size, raw_gap_size], as Ntjoin.format_paths returns it.
adjust(paths, no_cut, G) -> (paths, source): the adjusted rows per path, and per output row the (path, node) of the input row it is
(the head of its merged chain).  Where ntJoin would raise KeyError (a segment removed from a contig's set twice), KeyError((path,
node)) names the input row whose merge step found the segment gone."""

CONTIG, ORI, START, END, SIZE, FIRST_MX, TERMINAL_MX, GAP, RAW_GAP = range(9)


class Node:
    "one path node: mutable, shared between the lists that hold it"

    def __init__(self, row, where):
        (self.contig, self.ori, self.start, self.end, self.size, self.first_mx, self.terminal_mx, self.gap, self.raw_gap) = row
        self.where = where

    def length(self):
        return self.end - self.start

    def row(self):
        return [self.contig, self.ori, self.start, self.end, self.size, self.first_mx, self.terminal_mx, self.gap, self.raw_gap]


def intersects(a, b):
    "bedtools' rule for two half-open intervals (start, end) of one contig"
    return max(a[0], b[0]) < min(a[1], b[1])


def region_blocked(start, end, node_i, node_j, segments):
    """a segment of the contig's set touches [start, end] (closed) and shares neither its start nor its end with node_i, and neither
    with node_j"""
    for s, e in segments:
        if start <= e and s <= end and s != node_i.start and e != node_i.end and s != node_j.start and e != node_j.end:
            return True
    return False


def _take(segments, seg, node):
    if seg not in segments:
        raise KeyError(node.where)
    segments.remove(seg)


def merge_relocations(path, sets):
    "adjacent nodes of one contig, both '+' and ascending or both '-' and descending, become one unless a foreign segment is in the way"
    if len(path) < 2:
        return path
    out = [path[0]]
    for node_i, node_j in zip(path, path[1:]):
        if node_i.contig != node_j.contig:
            out.append(node_j)
            continue
        segments, head = sets[node_i.contig], out[-1]
        if node_i.ori == "+" and node_j.ori == "+" and node_i.end <= node_j.start:
            if region_blocked(node_i.start, node_j.end, node_i, node_j, segments):
                out.append(node_j)
                continue
            segments.add((head.start, node_j.end))
            _take(segments, (head.start, head.end), node_j)
            _take(segments, (node_j.start, node_j.end), node_j)
            head.end, head.terminal_mx, head.gap = node_j.end, node_j.terminal_mx, node_j.gap
        elif node_i.ori == "-" and node_j.ori == "-" and node_i.start >= node_j.end:
            if region_blocked(node_j.start, node_i.end, node_i, node_j, segments):
                out.append(node_j)
                continue
            segments.add((node_j.start, head.end))
            _take(segments, (head.start, head.end), node_j)
            _take(segments, (node_j.start, node_j.end), node_j)
            head.start, head.first_mx, head.gap = node_j.start, node_j.first_mx, node_j.gap
        else:
            out.append(node_j)
    return out


def is_best_region(regions, query):
    "query is as long as the first longest of the contig's nodes and ends on the same minimizer"
    best = None
    for node in regions:
        if node.length() > (best.length() if best is not None else 0):
            best = node
    return query.length() == (best.length() if best is not None else 0) and best.terminal_mx == query.terminal_mx


def is_subsumed(i, path, regions):
    if i == 0 or i >= len(path) - 1:
        return False
    prev, nxt = path[i - 1], path[i + 1]
    return (prev.contig == nxt.contig and prev.ori == nxt.ori and min(prev.start, nxt.start) == 0
            and max(prev.end, nxt.end) == prev.size and len(regions[prev.contig]) == 2)


def no_cut_paths(paths, sets, G):
    regions = {}
    for path in paths:
        for node in path:
            regions.setdefault(node.contig, []).append(node)
    middle = []
    for path in paths:
        kept = [node for i, node in enumerate(path) if not is_subsumed(i, path, regions)]
        middle.append(merge_relocations(kept, sets))
    out = []
    for path in middle:
        new = []
        for i, node in enumerate(path):
            n = len(regions[node.contig])
            if (n > 1 and is_best_region(regions[node.contig], node)) or (n == 1 and node.length() < node.size):
                node.start, node.end = 0, node.size
                new.append(node)
            elif n > 1:
                if 0 < i < len(path) - 1 and new:
                    new[-1].gap += node.length()
                    if G > 0:
                        new[-1].gap = min(G, new[-1].gap)
            else:
                new.append(node)
        out.append(new)
    return out


def closed_overlap(a, b):
    return a[0] <= b[1] and b[0] <= a[1]


def inside(a, b):
    return a[0] >= b[0] and a[1] <= b[1]


def find_non_overlapping(regions):
    """regions: a contig's segments that intersect another one, ascending -> {segment: its replacement or None}.  The longest (the
    first of them) stays; the others are dropped when inside it, cut back when they reach into it; then neighbours in ascending
    order are compared, each sweep on the values it started with, until a sweep finds no overlap"""
    best = None
    for seg in regions:
        if best is None or seg[1] - seg[0] > best[1] - best[0]:
            best = seg
    after = {}
    for seg in regions:
        if seg == best:
            after[seg] = seg
        elif inside(seg, best):
            after[seg] = None
        elif closed_overlap(seg, best):
            after[seg] = (seg[0], best[0] - 1) if seg[0] <= best[0] else (best[1] + 1, seg[1])
        else:
            after[seg] = seg
    again = True
    while again:
        again = False
        order = sorted(((b, a) for b, a in after.items() if a is not None), key=lambda x: x[1])  # stable: ties keep insertion order
        for (b1, a1), (b2, a2) in zip(order, order[1:]):
            if not closed_overlap(a1, a2):
                continue
            again = True
            if inside(a1, a2):
                after[b1] = None
            elif inside(a2, a1):
                after[b2] = None
            elif a1[1] - a1[0] > a2[1] - a2[0]:
                after[b2] = (a1[1] + 1, a2[1])
            else:
                after[b1] = (a1[0], a2[0] - 1)
    return after


def intersection_counts(segments):
    "per segment, in (start, end) ascending order: how many segments of the list it intersects (itself included)"
    order = sorted(segments)
    return [(seg, sum(intersects(seg, other) for other in order)) for seg in order]


def intersecting_regions(sets):
    out = {}
    for contig, segments in sets.items():
        hit = [seg for seg, count in intersection_counts(segments) if count > 1]
        if hit:
            out[contig] = find_non_overlapping(hit)
    return out


def remove_overlapping(path, fixes):
    out = []
    for node in path:
        table = fixes.get(node.contig)
        seg = (node.start, node.end)
        if table is not None and seg in table:
            new = table[seg]
            if new is None:
                continue
            node.start, node.end = new
        out.append(node)
    return out


def adjust(paths, no_cut=False, G=0, trace=None):
    "trace: a dict that receives the contigs' segment sets as phase 4 sees them"
    paths = [[Node(row, (p, i)) for i, row in enumerate(path)] for p, path in enumerate(paths)]
    sets = {}
    for path in paths:  # phase 1
        if len(path) >= 2:
            for node in path:
                sets.setdefault(node.contig, set()).add((node.start, node.end))
    paths = [merge_relocations(path, sets) for path in paths]  # phase 2
    if no_cut:
        paths = no_cut_paths(paths, sets, G)  # phase 3
    if trace is not None:
        trace["sets"] = {contig: set(segments) for contig, segments in sets.items()}
    fixes = intersecting_regions(sets)  # phase 4
    out = []
    for path in paths:
        path = merge_relocations(path, sets)  # phase 5
        path = remove_overlapping(path, fixes)  # phase 6
        for node in reversed(path):  # phase 7
            if node.ori != "?":
                node.gap = 0
                break
        out.append(path)
    return [[node.row() for node in path] for path in out], [[node.where for node in path] for path in out]
