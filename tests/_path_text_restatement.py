"""The .path and AGP text restated in plain Python: the contract of mxg_write_paths (include/ntjoin_mx.h) as
executable text.  Two restatements of the same files:

  by_regex   the loop of Ntjoin.print_scaffolds as it stood before the library wrote these files (reference
             bin/ntjoin_assemble.py:605-610), with write_agp's round trip through two regular expressions per component (:346-376);
  direct     every line formatted from the node's fields, as the kernels do it, with no string parsed back.

tests/test_path_text_cpu.py holds the two against each other (so the device may skip the round trip) and by_regex against the
goldens.  Both work on plain rows and strips and need no engine.  A path is a list of nodes (id, ori, start, end, gap_size,
start_adjust, end_adjust), as tests/_scaffold_restatement.py takes them; leads / tails are the strips of mxg_write_scaffolds, one
per path; unassigned = [(id, lo, hi, lead, tail)] per line of the BED, or None for no unassigned lines.  Test infrastructure only."""
import re


def path_coords(ori, start, end, start_adjust, end_adjust):
    "get_adjusted_start / get_adjusted_end of the reference's PathNode (bin/path_node.py:41-61)"
    length = end - start
    end_adj = length if end_adjust == 0 else end_adjust
    if ori == "+":
        return start + start_adjust, end - (length - end_adj)
    return start + (length - end_adj), end - start_adjust


def stripped(path, lead, tail):
    "[ori, start, end] per node with the strips applied to the end nodes (join_sequences :413-436)"
    coords = [[nd[1], nd[2], nd[3]] for nd in path]
    for c, strip, left in ((coords[0], lead, True), (coords[-1], tail, False)):
        if strip:
            if (c[0] == "+") == left:
                c[1] += strip
            else:
                c[2] -= strip
    return coords


def agp_of_path_string(scaffold_id, path_str):
    "write_agp (:346-376): one W line per contig component and one N line per gap of the path string"
    out, at, part = [], 1, 1
    for comp in path_str.split():
        ctg = re.search(r"(\S+)([\+\-])\:(\d+)-(\d+)", comp)
        gap = re.search(r"(\d+)N", comp)
        if ctg:
            c_start, c_end = int(ctg.group(3)) + 1, int(ctg.group(4))
            n = c_end - c_start + 1
            cols = (scaffold_id, at, at + n - 1, part, "W", ctg.group(1), c_start, c_end, ctg.group(2))
        elif gap:
            n = int(gap.group(1))
            cols = (scaffold_id, at, at + n - 1, part, "N", n, "scaffold", "yes", "align_genus")
        else:
            raise ValueError("Path string is not formatted correctly: " + path_str)
        out.append("\t".join(str(c) for c in cols) + "\n")
        at += n
        part += 1
    return "".join(out)


def agp_unassigned(unassigned):
    "write_agp_unassigned (:379-404): every interval that keeps text behind its strips"
    out = []
    for ctg, lo, hi, lead, tail in unassigned or []:
        n = hi - lo - lead - tail
        if n <= 0:
            continue
        start = lo + 1 + lead
        out.append("\t".join(str(c) for c in (f"{ctg}:{lo}-{hi}", 1, n, 1, "W", ctg, start, start + n - 1, "+")) + "\n")
    return "".join(out)


def by_regex(paths, leads, tails, first_line, unassigned=None):
    "-> (.path text, AGP text)"
    text, agp = [first_line + "\n"], []
    for ct, (path, lead, tail) in enumerate(zip(paths, leads, tails)):
        parts = []
        for nd, (ori, start, end) in zip(path, stripped(path, lead, tail)):
            a_start, a_end = path_coords(ori, start, end, nd[5], nd[6])
            parts.append(f"{nd[0]}{ori}:{a_start}-{a_end} {nd[4]}N")
        path_str = re.sub(r"\s+\d+N$", "", " ".join(parts))
        text.append(f"ntJoin{ct}\t{path_str}\n")
        agp.append(agp_of_path_string(f"ntJoin{ct}", path_str))
    return "".join(text), "".join(agp) + agp_unassigned(unassigned)


class Refused(Exception):
    "an input mxg_write_paths answers with MXG_EINVAL"


def direct(paths, leads, tails, first_line, unassigned=None):
    "-> (.path text, AGP text), every field placed where the kernels place it; Refused names `path <p> node <i>`"
    text, agp = [first_line + "\n"], []
    for p, (path, lead, tail) in enumerate(zip(paths, leads, tails)):
        if len(path) < 2:
            raise Refused(f"path {p} has {len(path)} node(s)")
        at, line = 1, []
        for i, (nd, (ori, start, end)) in enumerate(zip(path, stripped(path, lead, tail))):
            if nd[2] >= nd[3] or nd[6] > nd[3] - nd[2]:
                raise Refused(f"path {p} node {i}")
            s, e = path_coords(ori, start, end, nd[5], nd[6])
            if s < 0 or s >= e:
                raise Refused(f"path {p} node {i}: the adjusted interval is empty or inverted")
            last = i + 1 == len(path)
            line.append(f"{nd[0]}{ori}:{s}-{e}" + ("\n" if last else f" {nd[4]}N "))
            n = e - s
            agp.append(f"ntJoin{p}\t{at}\t{at + n - 1}\t{2 * i + 1}\tW\t{nd[0]}\t{s + 1}\t{e}\t{ori}\n")
            at += n
            if not last:
                agp.append(f"ntJoin{p}\t{at}\t{at + nd[4] - 1}\t{2 * i + 2}\tN\t{nd[4]}\tscaffold\tyes\talign_genus\n")
                at += nd[4]
        text.append(f"ntJoin{p}\t" + "".join(line))
    return "".join(text), "".join(agp) + agp_unassigned(unassigned)
