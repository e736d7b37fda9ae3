"""Inputs of the scaffold stage's tests: the goldens as the restatement and the library take them, FASTA files of a given line
width, and the seeded fuzz cases (tests/test_scaffolds_cpu.py checks their coverage on the CPU, tests/test_gpu_scaffolds.py runs
them).  Test infrastructure only."""
import json
import os
import random

from tests import _scaffold_restatement as rs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FUZZ_SEEDS = list(range(1, 49))
MAX_LEFT_OUT = 0.05  # share of the generated paths (every draw counts) the fuzz may leave out because the restatement refuses them
TILE = 8192          # output bytes per work-group of k_scaf_emit (csrc/scaffold.hip SCAF_TILE)


def load_golden(path):
    with open(path, encoding="ascii") as fh:
        doc = json.load(fh)
    return doc, os.path.join(GOLDEN, "fasta", doc["meta"]["fasta"])


def golden_nodes(doc):
    "the golden's paths as print_scaffolds holds them at :580: '?' nodes and short paths dropped, the last gap zeroed, cuts attached"
    out = []
    for path, cuts in zip(doc["paths"], doc["adjust"]):
        nodes = [nd for nd in path if nd[1] != "?"]
        if len(nodes) < 2:
            continue
        assert len(cuts) == len(nodes)
        rows = [(nd[0], nd[1], nd[2], nd[3], nd[7], sa, ea) for nd, (sa, ea) in zip(nodes, cuts)]
        rows[-1] = rows[-1][:4] + (0,) + rows[-1][5:]
        out.append(rows)
    return out


def rows_of(paths, index):
    "paths of restatement nodes -> rows for MxEngine.write_scaffolds, path_first"
    rows, first = [], [0]
    for path in paths:
        rows.extend((index[c], s, e, g, sa, ea, o == "-") for c, o, s, e, g, sa, ea in path)
        first.append(len(rows))
    return rows, first


def write_fasta(path, records, width=60, final_newline=True):
    "width 0: every record on one line"
    lines = []
    for rid, seq in records:
        lines.append(">" + rid)
        lines.extend([seq] if not width else [seq[i:i + width] for i in range(0, len(seq), width)])
    with open(path, "w", encoding="ascii", newline="") as fh:
        fh.write("\n".join(lines) + ("\n" if final_newline else ""))


def fuzz_case(seed):
    """-> dict(records, paths, overlap_gap, fold, width, final_newline, features, generated, left_out).  Records are blocks of random
    text (plain, mixed case, IUPAC codes and U) and runs of N/n, some longer than an emit tile; node borders prefer block borders, so
    that pieces begin and end inside N runs; nodes share and overlap ranges; some records are N throughout, some untouched."""
    rng = random.Random(seed)
    feats = set()
    overlap_gap = None if seed % 2 else rng.choice([0, 20, 20, 33])
    fold = seed % 4 >= 2
    width = [50, 60, 80, 0][seed % 4] if seed % 8 < 4 else rng.choice([50, 60, 80, 0, 7])
    final_newline = seed % 3 != 0
    feats |= {f"width{width}", "fold" if fold else "nofold", "overlap_on" if overlap_gap is not None else "overlap_off",
              "final_newline" if final_newline else "no_final_newline"}
    records, borders = [], []
    for r in range(rng.randint(3, 7)):
        blocks, cuts, at = [], [0], 0
        for _ in range(rng.randint(2, 7)):
            kind = rng.random()
            if kind < 0.3:
                n = rng.choice([1, 2, 5, 40, 64, 65, 300, TILE + 17, 2 * TILE + 100]) if rng.random() < 0.8 else rng.randint(1, 3 * TILE)
                blocks.append("".join(rng.choice("NNNn") for _ in range(n)))
                if n > TILE:
                    feats.add("n_run_longer_than_tile")
            else:
                alphabet = rng.choice(["ACGT", "ACGTacgt", "ACGTUacgtuRYKMSWBDHVNrykmswbdhvn", "ACGTU", "ACGTN"])
                if len(alphabet) > 8:
                    feats.add("iupac_mixed_case")
                blocks.append("".join(rng.choice(alphabet) for _ in range(rng.randint(1, 4000))))
            at += len(blocks[-1])
            cuts.append(at)
        records.append((f"r{r}", "".join(blocks)))
        borders.append(cuts)
    records.append(("allN", "N" * rng.choice([1, 63, 64, 1000])))
    borders.append([0, len(records[-1][1])])
    records.append(("untouched", "".join(rng.choice("ACGTn") for _ in range(rng.randint(1, 500)))))
    feats |= {"record_all_n", "record_untouched"}
    seqs = dict(records)
    usable = len(records) - 1  # (everything but "untouched"; "allN" only ever as a middle node)

    valid = [[i for i, c in enumerate(seq) if c not in "Nn"] for _, seq in records]

    def node(middle):
        "an end node (first or last of a path) is built around a base that is not N and that its cuts keep: the contract refuses others"
        r = rng.randrange(usable if middle else usable - 1)
        while not middle and not valid[r]:
            r = rng.randrange(usable - 1)
        rid, seq = records[r]
        ori = rng.choice("+-")
        if middle:
            pick = lambda: rng.choice(borders[r]) if rng.random() < 0.6 else rng.randint(0, len(seq))  # noqa: E731
            a, b = pick(), pick()
            if a == b:
                a, b = 0, len(seq)
            start, end = min(a, b), max(a, b)
            keep = None
        else:
            q = rng.choice(valid[r])
            start = rng.choice([x for x in borders[r] if x <= q]) if rng.random() < 0.6 else rng.randint(0, q)
            end = rng.choice([x for x in borders[r] if x > q]) if rng.random() < 0.6 else rng.randint(q + 1, len(seq))
            keep = q - start if ori == "+" else end - 1 - q
        length = end - start
        sa = ea = 0
        if overlap_gap is not None:
            sa = rng.choice([0, rng.randint(0, length if keep is None else keep)])
            ea = rng.choice([0, rng.randint(1 if keep is None else keep + 1, length)])
            if middle and rng.random() < 0.15:
                ea = rng.randint(1, length)
                sa = rng.randint(ea, length)
        return (rid, ori, start, end, rng.choice([0, 0, 1, 20, 137]), sa, ea)

    paths, generated, left_out = [], 0, 0  # every draw counts as generated, every refused draw as left out
    for _ in range(rng.randint(3, 12)):
        n = rng.randint(2, 6)
        for _attempt in range(30):
            generated += 1
            path = [node(0 < i < n - 1) for i in range(n)]
            if rng.random() < 0.3:  # nodes that share or overlap a range
                if n > 2:
                    src = path[rng.randrange(n)]
                    path[rng.randrange(1, n - 1)] = (src[0], rng.choice("+-"), src[2], src[3], src[4], src[5], src[6])
                else:
                    path[1] = path[0]
            path[-1] = path[-1][:4] + (rng.choice([0, 0, 0, 5]),) + path[-1][5:]
            try:
                rs.scaffolds([path], seqs, overlap_gap)
            except rs.Refused:
                left_out += 1
                continue
            paths.append(path)
            break
    for path in paths:
        for c, o, s, e, g, sa, ea in path:
            feats.add("ori" + o)
            feats.add("gap0" if g == 0 else "gap")
            if overlap_gap is not None:
                feats.add(f"adjust_{int(sa > 0)}{int(ea > 0)}")
                if sa >= (ea if ea else e - s):
                    feats.add("start_adjust_beyond_end")
    used = sorted((c, s, e) for path in paths for c, _o, s, e, *_ in path)
    if any(a[0] == b[0] and b[1] < a[2] for a, b in zip(used, used[1:])):
        feats.add("overlapping_ranges")
    text, leads, tails = rs.scaffolds(paths, seqs, overlap_gap, fold)
    if any(leads) or any(tails):
        feats.add("strip")
    if any(x > TILE for x in leads + tails):
        feats.add("strip_longer_than_tile")
    return {"records": records, "paths": paths, "overlap_gap": overlap_gap, "fold": fold, "width": width, "final_newline": final_newline,
            "features": feats, "generated": generated, "left_out": left_out}


REQUIRED_FEATURES = {"width50", "width60", "width80", "width0", "fold", "nofold", "overlap_on", "overlap_off", "final_newline",
                     "no_final_newline", "n_run_longer_than_tile", "iupac_mixed_case", "record_all_n", "record_untouched", "ori+", "ori-",
                     "gap0", "gap", "adjust_00", "adjust_01", "adjust_10", "adjust_11", "start_adjust_beyond_end", "overlapping_ranges",
                     "strip", "strip_longer_than_tile"}
