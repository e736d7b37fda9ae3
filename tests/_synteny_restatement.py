"""A plain sequential restatement of mxg_synteny_blocks' contract (include/ntjoin_mx.h, row f12) over the arrays of mxg_get_graph
and a piece table: it sorts the vertices, rebuilds the list piece by piece, then walks it anchor by anchor.  It shares no code with
the route (ntjoin_amd/csrc/synteny.h, synteny.hip).  Test infrastructure only: no GPU, no library."""

FWD, REV, GAP = 0, 1, 2
FIELDS = ("n_anchors", "q_record", "q_start", "q_end", "s_record", "s_start", "s_end", "reverse")


def anchor_list(vpos, vrec, q, s, k, pieces=None, first=None):
    """-> [(qrec, qpos', srec, spos)] in list order.  vpos / vrec: [assembly][vertex] (get_graph's vertex_pos / vertex_record);
    pieces: rows (record, start, end, kind) with first: n_records + 1 offsets, or None"""
    nv = len(vpos[q]) if len(vpos) else 0
    base = sorted((int(vrec[q][v]), int(vpos[q][v]), int(vrec[s][v]), int(vpos[s][v])) for v in range(nv))
    if pieces is None:
        return base
    by_rec = {}
    for a in base:
        by_rec.setdefault(a[0], []).append(a)
    out = []
    for r in range(len(first) - 1):
        off = 0
        for rec, lo, hi, kind in ([int(x) for x in row] for row in pieces[int(first[r]):int(first[r + 1])]):
            if kind == FWD:
                for _qr, qp, sr, sp in by_rec.get(rec, ()):
                    if lo <= qp and qp + k <= hi:
                        out.append((r, off + (qp - lo), sr, sp))
            elif kind == REV:
                for _qr, qp, sr, sp in reversed(by_rec.get(rec, ())):
                    if lo <= qp and qp + k <= hi:
                        out.append((r, off + (hi - (qp + k)), sr, sp))
            off += hi - lo
    return out


def link(a, b, max_gap):
    "the direction (+1 / -1) of the link between neighbouring anchors a and b, or 0"
    if a[0] != b[0] or a[2] != b[2] or a[3] == b[3]:
        return 0
    if max_gap > 0 and (b[1] - a[1] > max_gap or abs(b[3] - a[3]) > max_gap):
        return 0
    return 1 if b[3] > a[3] else -1


def blocks(anchors, k, max_gap, min_anchors, min_span):
    "-> (kept blocks as tuples in FIELDS order, number of links)"
    n = len(anchors)
    links = [link(anchors[i], anchors[i + 1], max_gap) for i in range(n - 1)]
    out, j = [], 0
    while j < n - 1:
        d = links[j]
        if d == 0:
            j += 1
            continue
        r = 1
        while j + r < n - 1 and links[j + r] == d:
            r += 1
        a, b = anchors[j], anchors[j + r]
        blk = (r + 1, a[0], a[1], b[1] + k, a[2], min(a[3], b[3]), max(a[3], b[3]) + k, 1 if d < 0 else 0)
        if blk[0] >= min_anchors and blk[3] - blk[2] >= min_span:
            out.append(blk)
        j += r
    return out, sum(1 for d in links if d)


def synteny(vpos, vrec, q, s, k, max_gap=0, min_anchors=2, min_span=0, pieces=None, first=None):
    "-> dict(n_anchors_total, n_links, blocks: tuples in FIELDS order), as MxEngine.synteny_blocks reports them"
    anchors = anchor_list(vpos, vrec, q, s, k, pieces, first)
    kept, n_links = blocks(anchors, k, max_gap, min_anchors, min_span)
    return {"n_anchors_total": len(anchors), "n_links": n_links, "blocks": kept}


def query_lengths(lengths, pieces=None, first=None):
    "the lengths of the query's records: the handle's, or the sums of a table's pieces"
    if pieces is None:
        return [int(x) for x in lengths]
    return [sum(int(row[2]) - int(row[1]) for row in pieces[int(first[r]):int(first[r + 1])]) for r in range(len(first) - 1)]


def paf_line(blk, qname, qlen, tname, tlen, k):
    n, _qr, qs, qe, _sr, ss, se, rev = blk
    cols = (qname, qlen, qs, qe, "-" if rev else "+", tname, tlen, ss, se, min(n * k, qe - qs, se - ss), max(qe - qs, se - ss), 255, f"cm:i:{n}")
    return "\t".join(str(c) for c in cols) + "\n"


def paf(kept, qnames, qlens, tnames, tlens, k):
    return "".join(paf_line(b, qnames[b[1]], qlens[b[1]], tnames[b[4]], tlens[b[4]], k) for b in kept)
