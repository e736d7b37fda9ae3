"""Generated FASTA shapes for the assembly report (tests/test_seqreport_cpu.py, tests/test_gpu_report.py).  The unit that can go wrong
is a 4096-byte tile of the file's text (headers included: the device ingest keeps the file as it is), so the shapes are small and
place their N runs by file offset.  window_shapes() does the same for the scaffold files' window route
(tests/test_gpu_report_windows.py): nodes and records whose OUTPUT files, as tests/_scaffold_restatement.py writes them, hold their
features at given offsets."""
import random
import re
import string

from tests import _scaffold_restatement as rs

TILE = 4096
MIN_GAP = 10


def bases(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def one_line(header, seq):
    return f">{header}\n{seq}\n"


def place(rng, header, total, runs, fill="ACGT"):
    """a one-line record of `total` bases whose N runs lie at the given FILE offsets [lo, hi) when the record opens the file"""
    off = len(header) + 2
    seq = list(bases(rng, total, fill))
    for lo, hi in runs:
        assert lo >= off and hi - off <= total
        seq[lo - off:hi - off] = "N" * (hi - lo)
    # the bases around a run are no N, so the runs are exactly what was asked for
    return one_line(header, "".join(seq))


def wrapped(header, seq, width=60, eol="\n"):
    return f">{header}{eol}" + "".join(seq[i:i + width] + eol for i in range(0, len(seq), width))


def shapes():
    rng = random.Random(20)
    out = {}
    out["run_of_min_gap_minus_1_and_min_gap"] = one_line("a", bases(rng, 700) + "N" * (MIN_GAP - 1) + bases(rng, 600) + "N" * MIN_GAP + bases(rng, 800))
    out["run_ends_on_last_byte_of_tile_and_next_starts_on_first"] = place(rng, "a", 3 * TILE, [(TILE - 20, TILE), (2 * TILE, 2 * TILE + 15)])
    half = MIN_GAP // 2
    out["two_half_runs_across_tile_border_joined"] = place(rng, "a", 2 * TILE, [(TILE - half, TILE + half)])
    out["two_half_runs_across_tile_border_base_between"] = place(rng, "a", 2 * TILE, [(TILE - half - 1, TILE - 1), (TILE, TILE + half)])
    for eol, tag in (("\n", "lf"), ("\r\n", "crlf")):
        text = ""
        for phase in range(60):
            seq = bases(rng, 120 + phase) + "N" * 25 + bases(rng, 90)
            text += wrapped(f"p{phase}", seq, 60, eol)
        out[f"run_cut_by_line_end_at_every_phase_{tag}"] = text
    out["run_across_three_whole_tiles"] = one_line("a", bases(rng, 1000) + "N" * (3 * TILE + 700) + bases(rng, 900)) + \
        wrapped("b", bases(rng, 300) + "N" * (3 * TILE + 5) + bases(rng, 600))
    out["record_n_throughout"] = one_line("a", bases(rng, 600)) + one_line("gap", "N" * 50) + one_line("short", "N" * 5) + one_line("b", bases(rng, 700))
    out["record_begins_and_ends_with_gap"] = one_line("a", "N" * 12 + bases(rng, 800) + "n" * 30) + one_line("b", "NNN" + bases(rng, 20) + "NN")
    out["records_of_1_to_50_bases"] = "".join(one_line(f"r{i}", bases(rng, 1 + i % 50, "ACGTN")) for i in range(400))
    out["empty_records"] = ">e0\n" + one_line("a", bases(rng, 30)) + ">e1\n>e2\n" + one_line("b", "N" * 11) + ">e3\n"
    out["no_final_newline"] = one_line("a", bases(rng, 520)) + ">b\n" + bases(rng, 100) + "N" * 14
    out["lower_case_u_and_iupac"] = wrapped("a", bases(rng, 900, "ACGTacgtUuNnRYKMSWBDHVrykmswbdhv") + "n" * 12 + bases(rng, 700, "acgtu") + "nN" * 6 + "X*-.")
    return {k: v.encode() for k, v in out.items()}


def scan_depth():
    "enough 4096-byte items to pass every level of the scan at MXG_REPORT_SCAN_W=4 (more than 4 x 4 x 4 of them), N runs across many of them"
    rng = random.Random(21)
    text = ""
    for r in range(6):
        seq = ""
        for j in range(9):
            seq += bases(rng, rng.randint(500, 9000), "ACGTacgt") + "N" * rng.choice((1, 5, 9, 10, 11, 300, 4096, 9000))
        text += wrapped(f"s{r}", seq + bases(rng, 50)) if r % 2 else one_line(f"s{r}", seq)
    return text.encode()


WIN = 8192  # MXG_SCAF_WIN of the small-window runs: one emit tile


def scaffold_case():
    """hand-made nodes for mxg_write_scaffolds -> (records, paths, overlap_gap).  With the overlap stage on (gap 20):
    path 0: r0 (+, 5 N stripped from its left, 4 N at its right end) + 5 N of fill + r1 (3 N at its left): one run of 12;
    path 1: r2 reverse-complemented + 30 N + r3 cut at its left (start_adjust 37) + 20 N (its right is cut: the overlap gap) + r4
            cut at its right, whose last 10 bases are N and are stripped;
    path 2: part of r5 + r6 reversed; the rest of r5, all of r7 (N at both ends, a gap and lower case inside) and r8 (N throughout:
            in no file) are unassigned.
    The lengths make ">ntJoin1\\n" straddle byte 8192 of the assigned file and a run of exactly 10 N straddle byte 16384."""
    rng = random.Random(22)
    r0 = "NNNNN" + bases(rng, 3000) + "n" * 15 + bases(rng, 1000, "acgt") + bases(rng, 976) + "NNNN"
    r1 = "NNN" + bases(rng, 3175)
    r2 = bases(rng, 100) + "N" * 12 + bases(rng, 1888, "ACGTacgtRYKM") + "NNN" + bases(rng, 1997)
    r3 = list(bases(rng, 6000))
    r3[4190:4200] = "N" * 10
    r3 = "".join(r3)
    r4 = bases(rng, 2890) + "N" * 10 + bases(rng, 100)
    r5 = bases(rng, 100) + bases(rng, 800, "ACGTUu") + "n" * 11 + bases(rng, 300)
    r6 = bases(rng, 700) + "N" * 9 + bases(rng, 700)
    r7 = "NN" + bases(rng, 9000, "ACGTacgt") + "N" * 20 + bases(rng, 8000) + "nnn"
    r8 = "N" * 40
    records = [(f"r{i}", s) for i, s in enumerate((r0, r1, r2, r3, r4, r5, r6, r7, r8))]
    paths = [[("r0", "+", 0, len(r0), 5, 0, 0), ("r1", "+", 0, len(r1), 0, 0, 0)],
             [("r2", "-", 0, len(r2), 30, 0, 0), ("r3", "+", 0, len(r3), 7, 37, 5990), ("r4", "+", 0, len(r4), 0, 0, 2900)],
             [("r5", "+", 100, 900, 15, 0, 0), ("r6", "-", 0, len(r6), 0, 0, 0)]]
    return records, paths, 20


# ---- the window route of MXG_SCAF_REPORT: shapes placed by offset in the OUTPUT files
LANE, WAVE = 16, 1024  # bytes of text per thread and per wave of a 4096-byte item
FOLD_TOO = ("lower_and_fold",)  # the shapes that are also run with fold_case
GROWTH = (1, 3, 9, 27, 81, 243)  # N runs in six consecutive windows of lists_grow_three_times
ONE_CHAR_IDS = string.ascii_letters + string.digits


def byte_kinds(text):
    "per byte of FASTA text (one line a record): 0 = sequence text, 1 = passed over (a header's byte, a line end), 2 = a header's '>'"
    kinds, head = bytearray(len(text)), False
    for i, c in enumerate(text):
        if c == ">" and (i == 0 or text[i - 1] == "\n"):
            head, kinds[i] = True, 2
        elif head or c == "\n":
            kinds[i] = 1
        if c == "\n":
            head = False
    return kinds


def lane_masks(text):
    "-> [(valid, r)] per 16 bytes of the file: bit j of valid = byte j is sequence text, bit j of r = a record begins in front of byte j"
    kinds = byte_kinds(text)
    return [(sum(1 << j for j, k in enumerate(kinds[lo:lo + LANE]) if k == 0), sum(1 << j for j, k in enumerate(kinds[lo:lo + LANE]) if k == 2))
            for lo in range(0, len(kinds), LANE)]


def header_offsets(text):
    return [i for i, k in enumerate(byte_kinds(text)) if k == 2]


def n_runs(text):
    "[(offset, length)] of the N runs of a FASTA text (one line a record) or of bare sequence"
    blank = re.sub(">[^\\n]*", lambda m: " " * len(m.group()), text)
    return [(m.start(), m.end() - m.start()) for m in re.finditer("[Nn]+", blank)]


class _Unassigned:
    "records that no path uses, laid out by the offset their text gets in the unassigned FASTA (the two records of the one path go first)"

    def __init__(self, rng):
        self.rng, self.at = rng, 0
        self.records = [("p0", bases(rng, 40)), ("p1", bases(rng, 40))]
        self.paths = [[("p0", "+", 0, 40, 0, 0, 0), ("p1", "-", 0, 40, 0, 0, 0)]]

    def add(self, rid, seq):
        self.records.append((rid, seq))
        core = seq.strip("Nn")
        if core:  # (N throughout: in no file)
            self.at += len(f">{rid}:0-{len(seq)}\n") + len(core) + 1

    def fill_to(self, rid, target):
        "a record of plain bases behind which the file has `target` bytes: the next header's '>' is byte `target`"
        for pad in ("", "x", "xx"):
            for digits in range(1, 8):
                n = target - self.at - len(rid + pad) - 6 - digits
                if n >= 1 and len(str(n)) == digits:
                    self.add(rid + pad, bases(self.rng, n))
                    assert self.at == target
                    return
        raise AssertionError(f"no record ends at byte {target} from byte {self.at}")

    def case(self):
        _, text, _ = rs.unassigned(self.records, self.paths)
        assert len(text) == self.at
        return (self.records, self.paths, None), text


def _pair(rng, tag, total, gap=0, alphabet="ACGT"):
    "two records and the path that joins them into a scaffold of `total` bases, `gap` of them the N between the two"
    la = (total - gap) * 2 // 5
    a, b = bases(rng, la, alphabet), bases(rng, total - gap - la, alphabet)
    return [(tag + "a", a), (tag + "b", b)], [(tag + "a", "+", 0, len(a), gap, 0, 0), (tag + "b", "+", 0, len(b), 0, 0, 0)]


def _header_at_every_lane_phase(rng):
    u = _Unassigned(rng)
    for i in range(480):
        rid = "L" * 40 + str(i) if i % 5 == 0 else f"h{i}"  # (a header of 48 bytes and more covers at least two whole lanes)
        phase = (7 * i + 3) % LANE  # where the NEXT header's '>' falls
        for n in range(1 + 16 * (i % 3), 64):
            if (u.at + len(f">{rid}:0-{n}\n") + n + 1) % LANE == phase:
                break
        u.add(rid, bases(rng, n))
        assert u.at % LANE == phase
    case, text = u.case()
    offs, masks = header_offsets(text), lane_masks(text)
    assert all(sum(1 for o in offs if o % LANE == p) >= 20 for p in range(LANE))
    assert sum(1 for valid, r in masks if valid == 0 and r != 0) >= 10      # the '>' and nothing but header bytes (and a line end)
    assert sum(1 for valid, r in masks if valid == 0 and r == 0) >= 90      # in the middle of a header
    assert len(text) > 2 * WIN
    return case


def _several_borders_in_one_lane(rng):
    u = _Unassigned(rng)
    stripped = all_n = 0
    for i in range(520):
        rid = ONE_CHAR_IDS[i % len(ONE_CHAR_IDS)]
        if i % 13 == 5:
            seq = "N" * (1 + i % 4)  # N throughout: in the BED only
            all_n += 1
        elif i % 4 == 3:
            seq = bases(rng, 1 + i % 11, "ACGTN")
        else:
            seq = bases(rng, 1 + i % 3)
        if i % 7 == 2 and seq.strip("N"):
            seq = "N" + seq + "Nn"  # N at both ends: the file holds the stripped text, the header the whole range
            stripped += 1
        u.add(rid, seq)
    case, text = u.case()
    offs, masks = header_offsets(text), lane_masks(text)
    assert len(offs) >= 400 and stripped >= 50 and all_n >= 30
    assert ">a:0-1\n" in text and len(">a:0-1\nA\n") == 9
    assert sum(1 for _, r in masks if bin(r).count("1") >= 2) >= 30        # two borders in one lane
    assert {o % LANE for o in offs} == set(range(LANE))
    assert len(text) > TILE
    return case


def _header_across_lane_wave_tile_window(rng):
    u = _Unassigned(rng)
    # the '>' on the last byte in front of a lane, wave, tile and window border, and on the first byte behind one
    targets = [5 * LANE - 1, 9 * LANE, WAVE - 1, 2 * WAVE, TILE - 1, WIN - 1, 3 * TILE, 2 * WIN]
    for j, target in enumerate(targets):
        u.fill_to(f"f{j}", target)
        u.add(f"x{j}", bases(rng, 7))
    (records, paths, gap), text = u.case()
    offs = header_offsets(text)
    assert all(t in offs for t in targets)
    assert [(t + 1) % b for t, b in zip(targets[0::2][:3] + [targets[5]], (LANE, WAVE, TILE, WIN))] == [0, 0, 0, 0]
    assert [t % b for t, b in zip((targets[1], targets[3], targets[6], targets[7]), (LANE, WAVE, TILE, WIN))] == [0, 0, 0, 0]
    assert (targets[0] + 1) % WAVE and (targets[2] + 1) % TILE and (targets[4] + 1) % WIN and targets[6] % WIN  # (each border is of its own kind)
    # the assigned file: ">ntJoin1\n" with its '>' on byte W - 1, ">ntJoin2\n" with its '>' on byte 2 W
    paths = []
    for tag, total, fill in (("a", WIN - 1 - 10, 12), ("b", WIN + 1 - 10, 0), ("c", 220, 20)):
        recs, path = _pair(rng, tag, total, fill)
        records = records + recs
        paths.append(path)
    paths.append(u.paths[0])
    want = rs.scaffolds(paths, dict(records), gap)[0]
    assert want.index(">ntJoin1\n") == WIN - 1 and want.index(">ntJoin2\n") == 2 * WIN
    assert rs.unassigned(records, paths)[1] == text
    return records, paths, gap


def _header_longer_than_a_tile(rng):
    u = _Unassigned(rng)
    u.add("s0", bases(rng, 100) + "N" * 15 + bases(rng, 200))
    u.add("I" * 300, bases(rng, 260) + "N" * 12 + bases(rng, 240))
    u.add("J" * (2 * TILE + 50), bases(rng, 300) + "N" * 11 + bases(rng, 80))
    u.add("s1", bases(rng, 50))
    case, text = u.case()
    kinds = byte_kinds(text)
    whole = [t for t in range(0, len(kinds) - TILE + 1, TILE) if set(kinds[t:t + TILE]) == {1}]
    assert whole                                                             # a tile of header bytes only: no border, no base
    assert n_runs("".join(c for c, k in zip(text, kinds) if k == 0)) == [(100, 15), (575, 12), (1127, 11)]
    return case


def _run_from_pieces(rng):
    x = bases(rng, TILE - 13) + "NNN"                   # bytes [9, T - 1) of the assigned file
    y = "NNN" + bases(rng, TILE - 10) + "NNN"           # behind 3 N of fill: [T + 2, W - 2)
    z = "NNN" + bases(rng, 300)                         # behind 4 N of fill: from W + 2
    records = [("x", x), ("y", y), ("z", z), ("u", bases(rng, 30))]
    paths = [[("x", "+", 0, len(x), 3, 0, 0), ("y", "+", 0, len(y), 4, 0, 0), ("z", "+", 0, len(z), 0, 0, 0)]]
    want = rs.scaffolds(paths, dict(records), None)[0]
    assert n_runs(want) == [(TILE - 4, MIN_GAP - 1), (WIN - 5, MIN_GAP)]     # 3 + 3 + 3 across byte T, 3 + 4 + 3 across byte W
    assert want[TILE - 2] == want[TILE + 1] == "N" and want[WIN - 2] == want[WIN + 1] == "N"  # (the fill itself straddles the border)
    return records, paths, None


def _run_across_two_windows(rng):
    a = bases(rng, WIN + TILE - 100 - 9)                # the run begins at byte 12188, in the middle of window 1
    b = bases(rng, 2 * TILE - 7)                        # [7 T, 9 T - 7): tile 7 is plain
    c = "ACGTA" + "NN" + bases(rng, 400)
    records = [("a", a), ("b", b), ("c", c), ("u", bases(rng, 30))]
    paths = [[("a", "+", 0, len(a), 2 * WIN + 100, 0, 0), ("b", "-", 0, len(b), TILE + 7, 0, 0), ("c", "+", 0, len(c), 0, 0, 0)]]
    want = rs.scaffolds(paths, dict(records), None)[0]
    assert n_runs(want) == [(WIN + TILE - 100, 2 * WIN + 100), (9 * TILE - 7, TILE + 7), (10 * TILE + 5, 2)]
    assert set(want[2 * WIN:3 * WIN]) == {"N"}                               # one whole window of N
    assert want[7 * TILE - 1] == "N" and not set(want[7 * TILE:8 * TILE]) & set("N>\n")  # ends on a tile's last byte, a plain tile behind
    assert want[10 * TILE - 1] == "N" and "N" in want[10 * TILE:11 * TILE]   # the second one: the tile behind is not plain
    return records, paths, None


def _contig_across_windows(rng):
    recs0, path0 = _pair(rng, "a", 6 * WIN - 9 - 10)    # ">ntJoin1\n" is the last 9 bytes of window 5
    recs1, path1 = _pair(rng, "b", 5000)
    records, paths = recs0 + recs1, [path0, path1]
    want = rs.scaffolds(paths, dict(records), None)[0]
    assert "N" not in want and want.index(">ntJoin1\n") == 6 * WIN - 9 and len(recs0[0][1]) + len(recs0[1][1]) >= 5 * WIN
    return records, paths, None


def _lists_grow_three_times(rng):
    seq = bases(rng, WIN - 9)                           # the sequence's byte j is byte j + 9 of the assigned file
    for w, count in enumerate(GROWTH):
        part, at = list(bases(rng, WIN)), 20
        for i in range(count):
            n = 10 + i % 3
            part[at:at + n] = "N" * n
            at += n + 1 + i % 2
        assert at < WIN - 20
        seq = seq[:w * WIN - 9] + "".join(part) if w else "".join(part)[9:]
    seq += bases(rng, 100)
    records = [("a", seq[:10]), ("b", seq[10:]), ("u", bases(rng, 20))]
    paths = [[("a", "+", 0, 10, 0, 0, 0), ("b", "+", 0, len(seq) - 10, 0, 0, 0)]]
    want = rs.scaffolds(paths, dict(records), None)[0]
    for w, count in enumerate(GROWTH):
        runs = n_runs(want[w * WIN:(w + 1) * WIN])
        assert len(runs) == count and all(10 <= n <= 12 for _, n in runs)
        assert want[(w + 1) * WIN - 1] != "N" and want[(w + 1) * WIN] != "N"
    assert len(want) == 6 * WIN + 100 + 1 and 243 * 13 < WIN
    return records, paths, None


def _empty_files(rng, all_n):
    records, path = _pair(rng, "a", 700, 11)
    if all_n:
        records += [("n0", "N" * 30), ("n1", "n" * 5), ("n2", "Nn" * 2100)]
    assert rs.unassigned(records, [path])[1:] == ("", 0) and bool(rs.unassigned(records, [path])[0]) == all_n
    return records, [path], None


def _lower_and_fold(rng):
    mixed = "ACGTacgtUuRYKMSWBDHVrykmswbdhvNn"
    m = "a" + bases(rng, 3000, mixed) + "n" * 13 + bases(rng, 2000, mixed) + "U"
    q = "c" + bases(rng, 2000, "ACGTacgt") + "G"
    w = bases(rng, 900, mixed).strip("Nn")
    records = [("m", m), ("q", q), ("w", w)]
    paths = [[("m", "-", 0, len(m), 25, 0, 0), ("q", "+", 0, len(q), 0, 0, 0)]]
    asis, folded = (rs.scaffolds(paths, dict(records), None, fold)[0] for fold in (False, True))
    assert asis.startswith(">ntJoin0\nA") and "a" in asis and "u" not in asis[9:len(m)]  # (U's complement is A)
    assert folded == asis.upper().replace(">NTJOIN", ">ntJoin") and folded != asis
    return records, paths, None


def window_shapes():
    "name -> (records, paths, overlap_gap) for mxg_write_scaffolds; every builder asserts the offsets its shape is named for"
    rng = random.Random(23)
    out = {"header_at_every_lane_phase": _header_at_every_lane_phase(rng),
           "several_borders_in_one_lane": _several_borders_in_one_lane(rng),
           "header_across_lane_wave_tile_window": _header_across_lane_wave_tile_window(rng),
           "header_longer_than_a_tile": _header_longer_than_a_tile(rng),
           "run_from_pieces": _run_from_pieces(rng),
           "run_across_two_windows": _run_across_two_windows(rng),
           "contig_across_windows": _contig_across_windows(rng),
           "lists_grow_three_times": _lists_grow_three_times(rng),
           "empty_files_all_assigned": _empty_files(rng, False),
           "empty_files_unassigned_all_n": _empty_files(rng, True),
           "lower_and_fold": _lower_and_fold(rng)}
    return out


def window_texts(case, fold=False):
    "(assigned, unassigned) FASTA bytes the restatement expects of a case"
    records, paths, gap = case
    return rs.scaffolds(paths, dict(records), gap, fold)[0].encode(), rs.unassigned(records, paths)[1].encode()


def window_scan_depth():
    "a case whose assigned file has more than 4 x 4 x 4 items of 4096 bytes, N runs of every size inside the nodes and between them"
    rng = random.Random(24)
    records, paths = [], []
    for p in range(3):
        path = []
        for j in range(2):
            seq = ""
            for _ in range(9):
                seq += bases(rng, rng.randint(500, 9000), "ACGTacgt") + "N" * rng.choice((1, 5, 9, 10, 11, 300, 4096, 9000))
            rid = f"s{p}{j}"
            records.append((rid, seq + bases(rng, 50)))
            path.append((rid, "+-"[(p + j) % 2], 0, len(seq) + 50, (3, 5000, 12)[p] if j == 0 else 0, 0, 0))
        paths.append(path)
    records.append(("u", bases(rng, 700) + "N" * 40 + bases(rng, 900)))
    return records, paths, None


def line_end_tile():
    """a file whose second and third 4096-byte tile hold line ends only, inside an N run of 20 + 5: a tile without a base that is
    entered with an open run -- it must leave the run open"""
    rng = random.Random(25)
    text = ">a\n" + bases(rng, 100) + "N" * 20 + "\n" * (3 * TILE) + "N" * 5 + bases(rng, 50) + "\n"
    assert set(text[TILE:3 * TILE]) == {"\n"}
    return text.encode()
