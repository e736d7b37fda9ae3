"""Inputs of the scaffold stage's and the .path / AGP writer's pin to ntJoin's own print_scaffolds: the families that
tests/golden/make_golden_scaffold_fuzz.py records and that tests/test_scaffolds_cpu.py, tests/test_path_text_cpu.py,
tests/test_gpu_scaffolds.py and tests/test_gpu_path_writer.py re-make, the reader of tests/golden/scaffolds/families, and the
conditions of its README.  Plain Python: no GPU, no reference import.  Test infrastructure only.

A case is a dict(records, paths, overlap_gap, width, final_newline): records = [(id, text)], a path a list of nodes (id, ori, start,
end, gap_size, start_adjust, end_adjust) as tests/_scaffold_restatement.py takes them, overlap_gap None with the overlap stage off.
The paths are the generator's; zeroed() gives them as print_scaffolds holds them at :580 (the last gap 0), which is what the
library is handed."""
import functools
import hashlib
import json
import os
import random

from tests import _scaffold_cases as cases, _scaffold_restatement as rs

FAMILY_DIR = os.path.join(cases.GOLDEN, "scaffolds", "families")
FAMILIES = ("fuzz", "strip_beside_cuts", "agp_names")
TARGET = "t.fa.k15.w10.tsv"   # args.s of every recorded run: the .path file's first line is t.fa, the assigned FASTA t.fa.k15.w10.n1...
RUNS = (1, 63, 64, 65, 300, cases.TILE + 17)   # N runs an uncut end node of strip_beside_cuts begins or ends in
# the record ids of tests/test_gpu_path_writer.py RECORDS: 1, 2, 31, 32, 33 and 300 bytes, some of which look like the fields behind them
AGP_NAME_IDS = ["a", "b+", "c" * 27 + "+:1-", "d" * 32, "e-:7-9" + "e" * 27, "f" * 300]


# ---- generators ----------------------------------------------------------------------------------------------------------------------
def fuzz_case(seed):
    "tests/_scaffold_cases.py fuzz_case(seed), unchanged; the folded variant stays on the restatement (the reference folds no case)"
    case = cases.fuzz_case(seed)
    return {key: case[key] for key in ("records", "paths", "overlap_gap", "width", "final_newline")}


def _n_run(rng, n):
    return "".join(rng.choice("NNNn") for _ in range(n))


def _cut_node(rng, rid, length):
    "a node with both cuts and a gap that the overlap stage replaces; its piece begins and ends in the record's N-free flanks"
    start, end = rng.randint(0, 100), length - rng.randint(0, 100)
    return (rid, rng.choice("+-"), start, end, rng.choice([1, 20, 137]), rng.randint(1, 50), end - start - rng.randint(1, 50))


def strip_beside_cuts_case(end, ori, overlap_gap):
    """the overlap stage on; per run length of RUNS three paths: two nodes and four nodes with the `end` ("lead": first, "tail": last)
    node uncut, oriented `ori` and beginning (ending) in an N run of that length, and three nodes with both end nodes so; every other
    node carries both cuts and a gap > 0.  The records of the stripped nodes hold three more Ns outside the node's range."""
    rng = random.Random(f"strip_beside_cuts {end} {ori}")
    plain = "ACGTacgtRYKMSWrykmsw"
    records, lengths = [], {}
    for r in range(4):
        flank = ["".join(rng.choice(plain) for _ in range(200)) for _ in range(2)]
        middle = "".join(rng.choice("ACGTN") for _ in range(rng.randint(100, 600))) + _n_run(rng, rng.choice([0, 7, 300]))
        records.append((f"c{r}", flank[0] + middle + flank[1]))
    body = {}
    for n in RUNS:
        body[n] = rng.randint(200, 700)
        records.append((f"s{n}", _n_run(rng, n + 3) + "".join(rng.choice("ACGTacgt") for _ in range(body[n])) + _n_run(rng, n + 3)))
    lengths = {rid: len(seq) for rid, seq in records}

    def end_node(n, lead, o, gap):
        "uncut, oriented o; as the first node its piece begins with n Ns, as the last it ends with them"
        inner = rng.randint(3 + n + 50, 3 + n + body[n] - 50)   # the border that lies in the text
        if (o == "+") == lead:
            return (f"s{n}", o, 3, inner, gap, 0, 0)
        return (f"s{n}", o, inner, lengths[f"s{n}"] - 3, gap, 0, 0)

    def cut():
        rid = f"c{rng.randrange(4)}"
        return _cut_node(rng, rid, lengths[rid])

    paths = []
    for i, n in enumerate(RUNS):
        gap = [0, 5, 137][i % 3]
        for middle in (0, 2):
            rest = [cut() for _ in range(middle + 1)]
            paths.append([end_node(n, True, ori, gap)] + rest if end == "lead" else rest + [end_node(n, False, ori, 0)])
        other = RUNS[(i + 2) % len(RUNS)]
        paths.append([end_node(n if end == "lead" else other, True, ori, gap), cut(), end_node(other if end == "lead" else n, False, ori, 0)])
    return dict(records=records, paths=paths, overlap_gap=overlap_gap, width={"lead+": 60, "lead-": 0, "tail+": 80, "tail-": 7}[end + ori],
                final_newline=ori == "+")


def agp_names_case(cuts):
    "the six ids of AGP_NAME_IDS as first, middle and last node of two- and three-node paths; cuts: the overlap stage on, every node cut"
    rng = random.Random(f"agp_names {cuts}")
    records = [(rid, "".join(rng.choice("ACGTacgt") for _ in range(40 + 7 * r))) for r, rid in enumerate(AGP_NAME_IDS)]

    def node(r, gap):
        length = len(records[r][1])
        start, end = rng.randint(0, 5), length - rng.randint(0, 5)
        sa, ea = (rng.randint(1, 5), end - start - rng.randint(1, 5)) if cuts else (0, 0)
        return (AGP_NAME_IDS[r], rng.choice("+-"), start, end, gap, sa, ea)

    paths = []
    for i in range(6):
        for d in (0, 1, 3):
            paths.append([node(i, rng.choice([0, 1, 20, 137])), node((i + d) % 6, 0)])
        for d1, d2 in ((1, 2), (4, 0), (5, 3)):
            paths.append([node(i, rng.choice([1, 20])), node((i + d1) % 6, rng.choice([0, 9, 100])), node((i + d2) % 6, 0)])
    return dict(records=records, paths=paths, overlap_gap=20 if cuts else None, width=60, final_newline=True)


GENERATORS = {"fuzz_case": fuzz_case, "strip_beside_cuts_case": strip_beside_cuts_case, "agp_names_case": agp_names_case}


def family_specs():
    "family -> [(case name, generator, arguments)]: what the recorder records and the tests read back"
    return {
        "fuzz": [(f"seed{seed:02d}", "fuzz_case", dict(seed=seed)) for seed in cases.FUZZ_SEEDS],
        "strip_beside_cuts": [(f"{end}_{'fwd' if ori == '+' else 'rev'}", "strip_beside_cuts_case", dict(end=end, ori=ori, overlap_gap=gap))
                              for (end, ori), gap in zip((("lead", "+"), ("lead", "-"), ("tail", "+"), ("tail", "-")), (20, 0, 33, 20))],
        "agp_names": [("plain", "agp_names_case", dict(cuts=False)), ("cuts", "agp_names_case", dict(cuts=True))],
    }


# ---- a case's input and what the tests hand on ---------------------------------------------------------------------------------------
def case_digest(case):
    value = [[list(r) for r in case["records"]], [[list(nd) for nd in path] for path in case["paths"]], case["overlap_gap"], case["width"],
             case["final_newline"]]
    return hashlib.sha256(json.dumps(value, separators=(",", ":")).encode("ascii")).hexdigest()


def zeroed(paths):
    "the paths as print_scaffolds holds them at :580: the last node's gap 0 (check_terminal_node_gap_zero)"
    return [path[:-1] + [tuple(path[-1][:4]) + (0,) + tuple(path[-1][5:])] for path in paths]


def rows9(path):
    "a path as format_paths() gives it: [contig, ori, start, end, contig_size, first_mx, terminal_mx, gap_size, raw_gap_size] per node"
    return [[c, o, s, e, 0, "0", "0", g, g] for c, o, s, e, g, _sa, _ea in path]


def scaffold_digests(fasta_text):
    "the text of an assigned FASTA, every record on one line -> [[name, length, sha256 of the sequence line]]"
    lines = fasta_text.split("\n")
    assert lines[-1] == "" and len(lines) % 2 == 1 and all(line.startswith(">") for line in lines[:-1:2]), "not a one-line-per-record FASTA"
    return [[name[1:], len(seq), hashlib.sha256(seq.encode("ascii")).hexdigest()] for name, seq in zip(lines[:-1:2], lines[1:-1:2])]


@functools.lru_cache(maxsize=None)
def load_family(family):
    """-> {case name: golden entry with "case" (the input, re-made and checked against the recorded digest), "pinned" (the indexes of
    the paths the reference answered, in the order of its ntJoin<ct>), "paths" (those paths, the last gap zeroed), "path_lines" and
    "agp_lines" (the recorded text per pinned path; agp_lines a list of lines each)}.  Cached: read it, do not change it"""
    out = {}
    specs = family_specs()[family]
    for part in sorted(f for f in os.listdir(FAMILY_DIR) if f.startswith(family + ".") and f.endswith(".json")):
        with open(os.path.join(FAMILY_DIR, part), encoding="ascii") as fh:
            doc = json.load(fh)
        assert doc["meta"]["family"] == family
        for entry in doc["cases"]:
            meta = entry["meta"]
            case = GENERATORS[meta["generator"]](**meta["args"])
            assert case_digest(case) == meta["sha256"], f"{family}/{meta['name']}: the generator no longer gives the input the golden was recorded on"
            assert len(entry["status"]) == len(case["paths"])
            pinned = [p for p, status in enumerate(entry["status"]) if status == "ok"]
            lines = entry["path"].split("\n")
            assert lines[0] == TARGET[:4] and lines[-1] == "" and len(lines) == len(pinned) + 2 and len(entry["scaffolds"]) == len(pinned)
            agp_lines = [[] for _ in pinned]
            for line in entry["agp"].split("\n")[:-1]:
                name = line.split("\t", 1)[0]
                assert name.startswith("ntJoin")
                agp_lines[int(name[6:])].append(line)
            out[meta["name"]] = dict(entry, case=case, pinned=pinned, paths=[zeroed(case["paths"])[p] for p in pinned], path_lines=lines[1:-1],
                                     agp_lines=agp_lines)
    assert list(out) == [name for name, _g, _a in specs], f"{family}: the golden's cases are not those of family_specs()"
    return out


def all_cases():
    "[(family, case name)] of every recorded case, for parametrised tests"
    return [(family, name) for family in FAMILIES for name, _g, _a in family_specs()[family]]


def renumbered(entry, keep):
    "the recorded .path and AGP text of the pinned paths `keep` (positions among the pinned), numbered ntJoin0, ntJoin1, ... anew"
    text, agp = [TARGET[:4] + "\n"], []
    for ct, q in enumerate(keep):
        old = f"ntJoin{q}\t"
        assert entry["path_lines"][q].startswith(old) and all(line.startswith(old) for line in entry["agp_lines"][q])
        text.append(f"ntJoin{ct}\t" + entry["path_lines"][q][len(old):] + "\n")
        agp.extend(f"ntJoin{ct}\t" + line[len(old):] + "\n" for line in entry["agp_lines"][q])
    return "".join(text), "".join(agp)


def refused_nodes(entry):
    "{position among the pinned paths: its lowest node whose recorded interval is empty or inverted}: what mxg_write_paths refuses"
    out = {}
    for q, line in enumerate(entry["path_lines"]):
        bad = [i for i, (s, e) in enumerate(recorded_coords(line)) if s >= e]
        if bad:
            out[q] = bad[0]
    return out


def unassigned_intervals(case, paths):
    "[(id, lo, hi, lead, tail)] per line of the unassigned BED of `paths` (the complement as the restatement computes it; unpinned)"
    seqs = dict(case["records"])
    out = []
    for line in rs.unassigned(case["records"], paths)[0].splitlines():
        rid, lo, hi = line.split("\t")
        text = seqs[rid][int(lo):int(hi)]
        lead = len(text) - len(text.lstrip("Nn"))
        out.append((rid, int(lo), int(hi), lead, 0 if lead == len(text) else len(text) - len(text.rstrip("Nn"))))
    return out


# ---- what the reference answered: the counts behind the conditions of tests/golden/scaffolds/families/README.md ---------------------
def recorded_coords(line):
    "a recorded .path line -> [(start, end)] per node, read from behind the last ':' of every component (ids may hold anything)"
    out = []
    for comp in line.split("\t", 1)[1].split(" ")[::2]:
        start, end = comp.rsplit(":", 1)[1].split("-")
        out.append((int(start), int(end)))
    return out


def _unstripped(nd):
    "get_adjusted_start / get_adjusted_end (bin/path_node.py:47-61) of a node no strip has moved"
    _c, ori, start, end, _g, sa, ea = nd
    length = end - start
    e = ea if ea else length
    return (start + sa, end - (length - e)) if ori == "+" else (start + (length - e), end - sa)


def reference_strips(path, line):
    """(lead, tail) the reference stripped, from its own .path line: the first node's start ('+') or end ('-') and the last node's end
    ('+') or start ('-') against the node's coordinates; every other coordinate must be the unmoved one"""
    got, want = recorded_coords(line), [_unstripped(nd) for nd in path]
    assert len(got) == len(want)
    first, last = 0 if path[0][1] == "+" else 1, 1 if path[-1][1] == "+" else 0
    lead = abs(got[0][first] - want[0][first])
    tail = abs(got[-1][last] - want[-1][last])
    for i, (g, w) in enumerate(zip(got, want)):
        for side in (0, 1):
            if (i, side) not in ((0, first), (len(path) - 1, last)):
                assert g[side] == w[side], (line, i)
    return lead, tail


def _piece(seq, nd, overlap_gap):
    "get_fasta_segment and get_adjusted_sequence (:327-332, :519-527) of one node"
    _c, ori, start, end, gap, sa, ea = nd
    text = rs.oriented(seq, ori, start, end)
    if overlap_gap is None:
        return text + "N" * gap
    e = ea if ea else end - start
    return text[sa:e] + "N" * (0 if gap <= 0 else gap if e == end - start else overlap_gap)


def strip_on_a_cut_end_node(case, path, line):
    "the one reason the reference may raise for: overlap on, and the end node that :421 (first) or :436 (last) speaks of is cut and stripped"
    if case["overlap_gap"] is None or line not in (421, 436):
        return False
    nd = zeroed([path])[0][0 if line == 421 else -1]
    text = _piece(dict(case["records"])[nd[0]], nd, case["overlap_gap"])
    return bool(nd[5] or nd[6]) and bool(text) and (text[0] if line == 421 else text[-1]) in "Nn"


def counts(entries):
    "over a family's goldens, from the reference's answers and the inputs"
    c = dict(generated=0, raised=0, pinned=0, nodes=0, overlap_on=0, start_cut=0, end_cut=0, replaced_gap=0, start_beyond_end=0, lead=0, tail=0,
             long_strip=0, refused=0)
    for entry in entries.values():
        case = entry["case"]
        on = case["overlap_gap"] is not None
        c["generated"] += len(case["paths"])
        c["raised"] += len(case["paths"]) - len(entry["pinned"])
        for path, line in zip(entry["paths"], entry["path_lines"]):
            c["pinned"] += 1
            c["nodes"] += len(path)
            c["overlap_on"] += on
            for i, (_c, _o, start, end, gap, sa, ea) in enumerate(path):
                length = end - start
                c["start_cut"] += on and sa > 0
                c["end_cut"] += on and ea > 0
                c["replaced_gap"] += on and i + 1 < len(path) and gap > 0 and ea not in (0, length)
                c["start_beyond_end"] += on and sa >= (ea if ea else length)
            lead, tail = reference_strips(path, line)
            c["lead"] += lead > 0
            c["tail"] += tail > 0
            c["long_strip"] += max(lead, tail) > cases.TILE
            c["refused"] += any(s >= e for s, e in recorded_coords(line))
    return {key: int(value) for key, value in c.items()}


FUZZ_MINIMUMS = dict(pinned=300, nodes=1200, overlap_on=100, start_cut=200, end_cut=200, replaced_gap=90, start_beyond_end=50, lead=45, tail=40,
                     long_strip=30, refused=40)
FUZZ_MAX_RAISED = 0.15   # share of the generated paths the reference may leave unpinned, each for the one reason above


def check_conditions(family, entries):
    "the conditions that keep the pin from going hollow, from the recorded answers; -> the counts found"
    found = counts(entries)
    if family == "fuzz":
        for entry in entries.values():
            for p, status in enumerate(entry["status"]):
                if status != "ok":
                    err = status["error"]
                    assert err["type"] == "AssertionError" and strip_on_a_cut_end_node(entry["case"], entry["case"]["paths"][p], err["line"]), \
                        (entry["meta"]["name"], p, err)
        assert found["raised"] <= FUZZ_MAX_RAISED * found["generated"], found
        for name, least in FUZZ_MINIMUMS.items():
            assert found[name] >= least, (name, found)
        return found
    assert found["raised"] == 0, found
    if family == "strip_beside_cuts":
        assert found["pinned"] >= 40 and found["overlap_on"] == found["pinned"], found
        seen = {"lead": set(), "tail": set()}
        for entry in entries.values():
            for path, line in zip(entry["paths"], entry["path_lines"]):
                lead, tail = reference_strips(path, line)
                assert lead or tail
                for strip, nd, which in ((lead, path[0], "lead"), (tail, path[-1], "tail")):
                    if strip:
                        assert nd[5] == nd[6] == 0
                        seen[which].add((strip, nd[1]))
                stripped = [nd for nd, strip in ((path[0], lead), (path[-1], tail)) if strip]
                for i, nd in enumerate(path):   # every other node carries cuts, and a replaced gap unless it is the last
                    if nd not in stripped:
                        assert nd[5] > 0 and 0 < nd[6] < nd[3] - nd[2] and (nd[4] > 0 or i + 1 == len(path)), (entry["meta"]["name"], path)
        for which in ("lead", "tail"):
            assert seen[which] == {(n, o) for n in RUNS for o in "+-"}, (which, sorted(seen[which]))
        found["runs"] = sorted(RUNS)
        return found
    assert family == "agp_names"
    where = {"first": set(), "middle": set(), "last": set()}
    for entry in entries.values():
        for path in entry["paths"]:
            where["first"].add(path[0][0])
            where["last"].add(path[-1][0])
            where["middle"].update(nd[0] for nd in path[1:-1])
    assert all(ids == set(AGP_NAME_IDS) for ids in where.values()), where
    assert {len(path) for entry in entries.values() for path in entry["paths"]} == {2, 3}
    assert any(nd[5] for nd in entries["cuts"]["paths"][0]) and not any(nd[5] or nd[6] for path in entries["plain"]["paths"] for nd in path)
    return found
