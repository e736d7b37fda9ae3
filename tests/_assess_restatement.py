"""A plain sequential restatement of mxg_synteny_assess' contract (include/ntjoin_mx.h, row f13) over the kept blocks of a
mxg_synteny_blocks call: it walks the blocks one by one, sorts with sorted() and sums with Python's integers.  It shares no code with
the route (ntjoin_amd/csrc/assess.h, assess.hip, sort_kernels.h).  Test infrastructure only: no GPU, no library.

A block is a tuple in _synteny_restatement.FIELDS order: (n_anchors, q_record, q_start, q_end, s_record, s_start, s_end, reverse)."""

TRANSLOCATION, INVERSION, RELOCATION = 0, 1, 2
KINDS = ("translocation", "inversion", "relocation")
CHAIN_FIELDS = ("n_blocks", "first_block", "n_anchors", "q_record", "q_start", "q_end", "s_record", "s_start", "s_end", "reverse")
BP_FIELDS = ("chain", "kind", "at_join", "q_lo", "q_hi")
DEFAULTS = dict(merge_gap=100000, max_indel=1000, join_indel=100000)


def piece_of(pieces, first, r, x):
    "the index of the piece of record r that holds base x (GAP pieces count); without a table every record is one piece"
    if pieces is None:
        return 0
    off = 0
    rows = pieces[int(first[r]):int(first[r + 1])]
    for j, row in enumerate(rows):
        n = int(row[2]) - int(row[1])
        if off <= x < off + n:
            return j
        off += n
    return len(rows) - 1   # (a base outside the record: no block has one)


def at_join(a, b, pieces, first):
    return piece_of(pieces, first, a[1], a[3] - 1) != piece_of(pieces, first, a[1], b[2])


def joined(a, b, k, merge_gap, max_indel, join_indel, pieces=None, first=None):
    if (a[1], a[4], bool(a[7])) != (b[1], b[4], bool(b[7])):
        return False
    gq = b[2] - a[3]
    gs = (a[5] - b[6]) if a[7] else (b[5] - a[6])
    if gq < 1 - k or gs < 1 - k:
        return False
    if merge_gap > 0 and max(gq, gs) > merge_gap:
        return False
    bound = join_indel if at_join(a, b, pieces, first) else max_indel
    return not (bound > 0 and abs(gq - gs) > bound)


def nx_block(lengths, d):
    "{n50, l50, n75, l75, n90, l90} of a multiset of lengths against D"
    order = sorted((int(v) for v in lengths), reverse=True)
    out = {}
    for x in (50, 75, 90):
        nx = lx = total = 0
        if d > 0:
            for j, v in enumerate(order, 1):
                total += v
                if 100 * total >= x * d:
                    nx, lx = v, j
                    break
        out[f"n{x}"], out[f"l{x}"] = nx, lx
    return out


def covered(intervals):
    "the size of the union of half-open intervals (record, start, end), summed over the records"
    total, by_rec = 0, {}
    for r, lo, hi in intervals:
        by_rec.setdefault(r, []).append((lo, hi))
    for ivs in by_rec.values():
        reach = None
        for lo, hi in sorted(ivs):
            if reach is None or lo > reach:
                total += hi - lo
                reach = hi
            elif hi > reach:
                total += hi - reach
                reach = hi
    return total


def assess(blocks, k, q_len, s_len, merge_gap=100000, max_indel=1000, join_indel=100000, pieces=None, first=None):
    """-> dict as MxEngine.synteny_assess returns it, the arrays as lists: chains / bps are dicts of lists by CHAIN_FIELDS / BP_FIELDS"""
    blocks = [tuple(int(x) for x in b) for b in blocks]
    runs = []
    for i, b in enumerate(blocks):
        if i and joined(blocks[i - 1], b, k, merge_gap, max_indel, join_indel, pieces, first):
            runs[-1].append(i)
        else:
            runs.append([i])
    chains = []
    for run in runs:
        a, b = blocks[run[0]], blocks[run[-1]]
        chains.append((len(run), run[0], sum(blocks[i][0] for i in run), a[1], a[2], b[3], a[4], min(a[5], b[5]), max(a[6], b[6]), 1 if a[7] else 0))
    bps, counts = [], {(kind, j): 0 for kind in range(3) for j in range(2)}
    for c, (x, y) in enumerate(zip(chains, chains[1:])):
        if x[3] != y[3]:
            continue
        kind = TRANSLOCATION if x[6] != y[6] else INVERSION if x[9] != y[9] else RELOCATION
        j = 1 if at_join(blocks[x[1] + x[0] - 1], blocks[y[1]], pieces, first) else 0
        bps.append((c, kind, j, x[5], y[4]))
        counts[(kind, j)] += 1
    qb, sb = sum(int(v) for v in q_len), sum(int(v) for v in s_len)
    spans = [c[5] - c[4] for c in chains]
    return {
        "n_blocks": len(blocks), "n_chains": len(chains), "n_breakpoints": len(bps), "breakpoints": counts,
        "query_bases": qb, "subject_bases": sb, "aligned_query": sum(spans), "chained_subject": sum(c[8] - c[7] for c in chains),
        "covered_subject": covered([(c[6], c[7], c[8]) for c in chains]),
        "na": nx_block(spans, qb), "nga": nx_block(spans, sb), "ng": nx_block(q_len, sb),
        "chains": {name: [c[u] for c in chains] for u, name in enumerate(CHAIN_FIELDS)},
        "bps": {name: [b[u] for b in bps] for u, name in enumerate(BP_FIELDS)},
    }
