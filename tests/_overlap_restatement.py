"""The overlap stage's cut points restated in plain Python over the sketch oracle.  Test infrastructure only.

A path is a list of nodes (contig, ori, start, end, raw_gap) with ori in "+-" and at least two nodes; `seqs` maps a contig
to its text.  cuts() returns per path the lists start_adjust, end_adjust (per node, 0 = none) and cut_found (per node: the
junction to the next node got a cut), plus per junction what kind of component won, for the goldens' own statistics."""
import re

_COMP = str.maketrans("ACGTUacgtu", "TGCAAtgcaa")


def segment_text(seq, ori, start, end):
    s = seq[start:end]
    return s.translate(_COMP)[::-1] if ori == "-" else s


def mask_coords(lens, gaps, k, w):
    "per node the hard-masked range [l, r) of its text (r = l: nothing masked)"
    out = []
    for i, n in enumerate(lens):
        l = -gaps[i - 1] + k + w if i > 0 and gaps[i - 1] < 0 else 0
        r = n + gaps[i] - k - w if gaps[i] < 0 else n
        if l > r:
            r = l
        out.append((l, r))
    return out


def node_minimizers(text, i, lens, gaps, sketch):
    "the node's minimizers in its overlapping ends, those whose hash occurs more than once among them dropped: [(hash, pos)]"
    kept = []
    for h, pos in sketch(text):
        if (i > 0 and pos < -gaps[i - 1]) or pos >= lens[i] + gaps[i]:
            kept.append((h, pos))
    count = {}
    for h, _ in kept:
        count[h] = count.get(h, 0) + 1
    return [(h, p) for h, p in kept if count[h] == 1]


def junction_cut(src, tgt, len_src, gap):
    """src / tgt: the two nodes' minimizer lists.  None, or (source pos, target pos, kind, run length, string order differs from
    numeric order at the run's ends)"""
    s_list = [(h, p) for h, p in src if p >= len_src + gap]
    t_list = [(h, p) for h, p in tgt if p < -gap]
    t_hashes = {h for h, _ in t_list}
    s_hashes = {h for h, _ in s_list}
    s_list = [(h, p) for h, p in s_list if h in t_hashes]
    t_list = [(h, p) for h, p in t_list if h in s_hashes]
    if not s_list:
        return None
    t_rank = {h: r for r, (h, _) in enumerate(t_list)}
    t_pos = dict(t_list)
    runs, cur = [], [0]
    for j in range(1, len(s_list)):
        if abs(t_rank[s_list[j][0]] - t_rank[s_list[j - 1][0]]) == 1:
            cur.append(j)
        else:
            runs.append(cur)
            cur = [j]
    runs.append(cur)
    best = None
    for run in runs:
        walk = [s_list[j] for j in run]
        differs = False
        if len(walk) > 1:
            a, b = walk[0][0], walk[-1][0]
            differs = (str(a) < str(b)) != (a < b)
            if str(a) > str(b):  # the walk starts at the end whose name is the smaller STRING
                walk = walk[::-1]
            mapped2 = abs(walk[0][1] - walk[-1][1]) + abs(t_pos[walk[0][0]] - t_pos[walk[-1][0]])
        else:
            mapped2 = 2
        mid_h, mid_p = walk[len(walk) // 2]
        # get_dist_from_end is handed the node's index for `ori`, so it answers -pos for both lists, whatever the orientation
        key = (mapped2, -(mid_p + t_pos[mid_h]), str(mid_h))
        cand = (key, mid_p, t_pos[mid_h], "run" if len(walk) > 1 else "single", len(walk), differs)
        if best is None or cand[0] > best[0]:
            best = cand
    return best[1:]


def cuts(paths, seqs, k, w, sketch):
    """sketch(text, k, w) -> [(out_hash, pos), ...] as `indexlr --long --pos` gives it for the text"""
    starts, ends, found, kinds = [], [], [], []
    for path in paths:
        assert len(path) >= 2 and all(nd[1] in "+-" for nd in path)
        lens = [nd[3] - nd[2] for nd in path]
        gaps = [nd[4] for nd in path]
        mxs = []
        for i, ((ctg, ori, start, end, _), (l, r)) in enumerate(zip(path, mask_coords(lens, gaps, k, w))):
            text = segment_text(seqs[ctg], ori, start, end)
            assert len(text.strip("Nn")) == len(text), "a segment begins or ends with N"
            text = text[:l] + "N" * (r - l) + text[r:]
            assert len(text) == lens[i]
            mxs.append(node_minimizers(text, i, lens, gaps, lambda t: sketch(t, k, w)))
        sa, ea, cf, kd = [0] * len(path), [0] * len(path), [False] * len(path), [None] * len(path)
        for i in range(len(path) - 1):
            if gaps[i] < 0:
                got = junction_cut(mxs[i], mxs[i + 1], lens[i], gaps[i])
                if got is not None:
                    ea[i], sa[i + 1], cf[i] = got[0], got[1], True
                    kd[i] = got[2:]
                else:
                    kd[i] = ("none", 0, False)
        starts.append(sa)
        ends.append(ea)
        found.append(cf)
        kinds.append(kd)
    return starts, ends, found, kinds


def path_string(nodes, start_adjust, end_adjust):
    """the reference's .path line for one path (print_scaffolds :605-607) from its nodes [contig, ori, start, end, ..., gap_size at
    index 7] and the adjustments, by path_node.py's four coordinate rules (:41-62)"""
    parts = []
    for nd, sa, ea in zip(nodes, start_adjust, end_adjust):
        ori, start, end = nd[1], nd[2], nd[3]
        length = end - start
        end_adj = length if ea == 0 else ea
        if ori == "+":
            a_start, a_end = start + sa, end - (length - end_adj)
        else:
            a_start, a_end = start + (length - end_adj), end - sa
        parts.append(f"{nd[0]}{ori}:{a_start}-{a_end} {nd[7]}N")
    line = " ".join(parts)
    return re.sub(r"\s+\d+N$", "", line)
