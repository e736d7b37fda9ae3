"""Generated FASTA shapes for the assembly report (tests/test_seqreport_cpu.py, tests/test_gpu_report.py).  The unit that can go wrong
is a 4096-byte tile of the file's text (headers included: the device ingest keeps the file as it is), so the shapes are small and
place their N runs by file offset."""
import random

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
