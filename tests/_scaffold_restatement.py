"""The scaffold stage restated in plain Python: the contract of mxg_write_scaffolds (include/ntjoin_mx.h) as
strings.  Test infrastructure only; tests/test_scaffolds_cpu.py holds it to the reference's own output (tests/golden/scaffolds).

A node is (contig, ori, start, end, gap_size, start_adjust, end_adjust) with ori in "+-"; a path has at least two nodes; `records`
is the target as an ordered list of (id, text) with the text free of line ends.  Inputs the library refuses with MXG_EINVAL raise
Refused here."""
import re

_TABLE = str.maketrans("ACGTUNMRWSYKVHDBacgtunmrwsykvhdb", "TGCAANKYWSRMBDHVtgcaankywsrmbdhv")


class Refused(ValueError):
    "an input mxg_write_scaffolds answers with MXG_EINVAL"


def oriented(seq, ori, start, end):
    text = seq[start:end]
    return text[::-1].translate(_TABLE) if ori == "-" else text


def piece(seq, node, overlap_gap):
    "(text part, number of Ns behind it) of one node; overlap_gap None: the overlap stage is off"
    ctg, ori, start, end, gap, sa, ea = node
    if not 0 <= start < end <= len(seq):
        raise Refused(f"[{start}, {end}) is not a segment of {ctg}")
    text = oriented(seq, ori, start, end)
    if overlap_gap is None:
        return text, gap
    length = end - start
    if ea > length:
        raise Refused("end_adjust beyond the segment")
    e = ea if ea else length
    return text[sa:e], (0 if gap <= 0 else gap if e == length else overlap_gap)


def scaffolds(paths, seqs, overlap_gap=None, fold=False):
    "-> (text of the assigned FASTA, lead_strip per path, tail_strip per path)"
    out, leads, tails = [], [], []
    for p, path in enumerate(paths):
        if len(path) < 2:
            raise Refused(f"path {p} has fewer than two nodes")
        parts = [piece(seqs[nd[0]], nd, overlap_gap) for nd in path]
        for text, _ in (parts[0], parts[-1]):
            if not text.strip("Nn"):
                raise Refused(f"path {p}: a first or last piece without text")
        pieces = [text + "N" * n for text, n in parts]
        first = pieces[0].lstrip("Nn")
        leads.append(len(pieces[0]) - len(first))
        pieces[0] = first
        last = pieces[-1].rstrip("Nn")
        tails.append(len(pieces[-1]) - len(last))
        pieces[-1] = last
        seq = "".join(pieces)
        out.append(f">ntJoin{p}\n{seq.upper() if fold else seq}\n")
    return "".join(out), leads, tails


def unassigned(records, paths):
    "-> (text of the BED, text of the unassigned FASTA, records in that FASTA)"
    used = {}
    for path in paths:
        for nd in path:
            used.setdefault(nd[0], []).append((nd[2], nd[3]))
    bed, fasta, n = [], [], 0
    for rid, seq in records:
        at, gaps = 0, []
        for lo, hi in sorted(used.get(rid, [])):
            if lo > at:
                gaps.append((at, lo))
            at = max(at, hi)
        if len(seq) > at:
            gaps.append((at, len(seq)))
        for lo, hi in gaps:
            bed.append(f"{rid}\t{lo}\t{hi}\n")
            text = seq[lo:hi].strip("Nn")
            if text:
                fasta.append(f">{rid}:{lo}-{hi}\n{text}\n")
                n += 1
    return "".join(bed), "".join(fasta), n


def path_text(assembly_fa, paths, leads, tails):
    """the .path file (print_scaffolds :546, :605-608): join_sequences (:413-436) has moved the first node's start (end when '-') by
    the lead strip and the last node's end (start when '-') by the tail strip before PathNode's coordinate rules
    (bin/path_node.py:37-61) are applied to the moved coordinates"""
    lines = [assembly_fa + "\n"]
    for p, (path, lead, tail) in enumerate(zip(paths, leads, tails)):
        coords = [[nd[1], nd[2], nd[3]] for nd in path]
        if lead:
            coords[0][1 if coords[0][0] == "+" else 2] += lead if coords[0][0] == "+" else -lead
        if tail:
            coords[-1][2 if coords[-1][0] == "+" else 1] += -tail if coords[-1][0] == "+" else tail
        parts = []
        for nd, (ori, start, end) in zip(path, coords):
            length = end - start
            e = nd[6] if nd[6] else length
            if ori == "+":
                a_start, a_end = start + nd[5], end - (length - e)
            else:
                a_start, a_end = start + (length - e), end - nd[5]
            parts.append(f"{nd[0]}{ori}:{a_start}-{a_end} {nd[4]}N")
        lines.append(f"ntJoin{p}\t" + re.sub(r"\s+\d+N$", "", " ".join(parts)) + "\n")
    return "".join(lines)
