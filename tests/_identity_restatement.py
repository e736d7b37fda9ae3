"""The contract of mxg_identity_segments (include/ntjoin_mx.h, row f14), restated as a plain dynamic program over the cells of
the band, one number per cell.  Nothing here is shared with the library's code (ntjoin_amd/csrc/identity.h keeps the band as bit
vectors); the tests compare the two."""

E = 16
MAX_SHIFT = 31
ALIGNED, SKIP_LEN, SKIP_SHIFT, SKIP_N = 0, 1, 2, 3
DEFAULT_MAX_SEG = 10000
INF = float("inf")


def byte_class(ch):
    """0..3 for A C G T/U in either case, 4 for any other base; line breaks are no bases and never get here."""
    return {"A": 0, "C": 1, "G": 2, "T": 3, "U": 3}.get(ch.upper(), 4)


def bases(text):
    """The bases of a record's sequence text: its characters that are no line breaks."""
    return text.replace("\n", "").replace("\r", "")


def classes(interval, reverse=False):
    c = [byte_class(ch) for ch in interval]
    if reverse:
        c = [3 - x if x < 4 else 4 for x in reversed(c)]
    return c


def full_distance(Q, S):
    """The unbanded unit-cost edit distance of two class lists."""
    prev = list(range(len(S) + 1))
    for i in range(1, len(Q) + 1):
        cur = [i] + [0] * len(S)
        for j in range(1, len(S) + 1):
            cur[j] = min(prev[j - 1] + (Q[i - 1] != S[j - 1]), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[len(S)]


def banded_distance(Q, S):
    """D[lq][ls] over the cells whose diagonal j - i lies in [min(0, d) - E, max(0, d) + E]; cells outside are +infinity.
    A row is kept by diagonal: entry t of row i is the cell (i, i + lo + t), so that its diagonal neighbour is entry t of the row
    above, its upper neighbour entry t + 1 of the row above and its left neighbour entry t - 1 of its own row."""
    lq, ls = len(Q), len(S)
    d = ls - lq
    lo, hi = min(0, d) - E, max(0, d) + E
    width = hi - lo + 1
    prev = None
    for i in range(lq + 1):
        cur = [INF] * (width + 1)   # (one more: the upper neighbour of the last diagonal, never a cell)
        for t in range(max(0, -(i + lo)), min(width, ls - i - lo + 1)):
            j = i + lo + t
            if i == 0 and j == 0:
                cur[t] = 0
                continue
            best = INF
            if i and j:
                best = prev[t] + (Q[i - 1] != S[j - 1])
            if i and prev[t + 1] + 1 < best:
                best = prev[t + 1] + 1
            if j and t and cur[t - 1] + 1 < best:
                best = cur[t - 1] + 1
            cur[t] = best
        prev = cur
    return prev[ls - lq - lo]


def segment(q_interval, s_interval, reverse=False, max_seg=DEFAULT_MAX_SEG):
    """(edits, status, saturated) of one segment, given the bases of its two intervals as they stand in their records."""
    lq, ls = len(q_interval), len(s_interval)
    assert lq >= 1 and ls >= 1 and max_seg >= 1
    if lq > max_seg or ls > max_seg:
        return (0, SKIP_LEN, 0)
    if abs(ls - lq) > MAX_SHIFT:
        return (0, SKIP_SHIFT, 0)
    Q, S = classes(q_interval), classes(s_interval, reverse)
    if 4 in Q or 4 in S:
        return (0, SKIP_N, 0)
    edits = banded_distance(Q, S)
    return (edits, ALIGNED, 1 if edits > abs(ls - lq) + 2 * E else 0)


def segment_of_records(q_records, s_records, seg, max_seg=DEFAULT_MAX_SEG):
    """The same for seg = (q_record, q_start, lq, s_record, s_start, ls, reverse) over lists of sequence texts (line breaks and all)."""
    qr, qs, lq, sr, ss, ls, rev = seg
    q, s = bases(q_records[qr]), bases(s_records[sr])
    assert qs + lq <= len(q) and ss + ls <= len(s)
    return segment(q[qs:qs + lq], s[ss:ss + ls], bool(rev), max_seg)


# ---- the segments of synteny blocks (mxg_synteny_identity) ------------------------------------------------------------------------------
BLOCK_FIELDS = ("n_aligned", "n_skip_len", "n_skip_shift", "n_skip_n", "n_saturated", "aligned_q", "aligned_s", "edits")
SUM_FIELDS = ("n_blocks", "n_segments") + BLOCK_FIELDS[:5] + ("block_q",) + BLOCK_FIELDS[5:]


def block_segments(anchors, k, max_gap, min_anchors, min_span):
    """The kept blocks of an anchor list [(qrec, qpos', srec, spos)] (tests/_synteny_restatement.anchor_list), each as
    (q_start, q_end, [segments (q_record, q_start, lq, s_record, s_start, ls, reverse)]): a maximal run of links of one direction,
    one segment per link and one tail segment of k bases at its last anchor."""
    def direction(a, b):
        if a[0] != b[0] or a[2] != b[2] or a[3] == b[3]:
            return 0
        if max_gap > 0 and (b[1] - a[1] > max_gap or abs(b[3] - a[3]) > max_gap):
            return 0
        return 1 if b[3] > a[3] else -1
    out, j, n = [], 0, len(anchors)
    while j + 1 < n:
        d = direction(anchors[j], anchors[j + 1])
        if d == 0:
            j += 1
            continue
        e = j + 1
        while e + 1 < n and direction(anchors[e], anchors[e + 1]) == d:
            e += 1
        run = anchors[j:e + 1]
        q_start, q_end = run[0][1], run[-1][1] + k
        if len(run) >= min_anchors and q_end - q_start >= min_span:
            segs = []
            for a, b in zip(run, run[1:]):
                if d > 0:
                    segs.append((a[0], a[1], b[1] - a[1], a[2], a[3], b[3] - a[3], 0))
                else:
                    segs.append((a[0], a[1], b[1] - a[1], a[2], b[3] + k, a[3] - b[3], 1))
            last = run[-1]
            segs.append((last[0], last[1], k, last[2], last[3], k, 0 if d > 0 else 1))
            out.append((q_start, q_end, segs))
        j = e
    return out


def synteny_identity(anchors, k, q_records, s_records, max_gap=0, min_anchors=2, min_span=0, max_seg=DEFAULT_MAX_SEG):
    """-> dict: the summary by SUM_FIELDS and "blocks": {field: [per kept block]} by BLOCK_FIELDS.  q_records / s_records: the
    sequence texts of the query's and the subject's records (line ends and all)."""
    q, s = [bases(t) for t in q_records], [bases(t) for t in s_records]
    per = {name: [] for name in BLOCK_FIELDS}
    n_segments = block_q = 0
    for q_start, q_end, segs in block_segments(anchors, k, max_gap, min_anchors, min_span):
        row = dict.fromkeys(BLOCK_FIELDS, 0)
        for qr, qs, lq, sr, ss, ls, rev in segs:
            assert qs + lq <= len(q[qr]) and ss + ls <= len(s[sr])
            edits, status, sat = segment(q[qr][qs:qs + lq], s[sr][ss:ss + ls], bool(rev), max_seg)
            row[("n_aligned", "n_skip_len", "n_skip_shift", "n_skip_n")[status]] += 1
            if status == ALIGNED:
                row["n_saturated"] += sat
                row["aligned_q"] += lq
                row["aligned_s"] += ls
                row["edits"] += edits
        for name in BLOCK_FIELDS:
            per[name].append(row[name])
        n_segments += len(segs)
        block_q += q_end - q_start
    out = {name: sum(per[name]) for name in BLOCK_FIELDS}
    out.update(n_blocks=len(per["edits"]), n_segments=n_segments, block_q=block_q, blocks=per)
    return out


def paf_tags(aligned_q, aligned_s, edits):
    "what MXG_PAF_IDENTITY appends to a block's PAF line, in front of its line end"
    text = f"\tal:i:{aligned_q}"
    if aligned_q > 0:
        den = max(aligned_q, aligned_s)
        text += f"\tNM:i:{edits}\tdv:f:" + ("1.0000" if edits >= den else "0.%04d" % (10000 * edits // den))
    return text


def per_100kbp(edits, aligned_q, aligned_s):
    "edits * 10^5 / max(aligned_q, aligned_s) in integers, two decimals (the identity table's last column)"
    den = max(aligned_q, aligned_s)
    if den == 0:
        return "0.00"
    v = edits * 10 ** 7 // den
    return f"{v // 100}.{v % 100:02d}"
