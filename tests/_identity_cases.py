"""Segment cases of mxg_identity_segments shared by tests/test_identity_cpu.py (tools/identity_check against the restatement) and
tests/test_gpu_identity.py (the device against the restatement).  A case is (name, query interval, subject interval as it stands in
its text, reverse, max_seg); HAND carries the expected (edits, status, saturated) as literals."""
import random

COMP = str.maketrans("ACGTUacgtu", "TGCAAtgcaa")


def revcomp(s):
    return s.translate(COMP)[::-1]


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


# (name, q, s, reverse, max_seg, (edits, status, saturated)); status 0 aligned, 1 length, 2 shift, 3 class 4
HAND = [
    ("equal", "ACGT", "ACGT", 0, 10000, (0, 0, 0)),
    ("one_substitution", "ACGT", "AGGT", 0, 10000, (1, 0, 0)),
    ("one_deletion", "ACGT", "ACT", 0, 10000, (1, 0, 0)),
    ("one_insertion", "ACT", "ACGT", 0, 10000, (1, 0, 0)),
    ("single_bases", "A", "C", 0, 10000, (1, 0, 0)),
    ("single_equal", "G", "G", 0, 10000, (0, 0, 0)),
    ("kitten", "GATTACA", "GCATGCT", 0, 10000, (4, 0, 0)),
    ("palindrome_reverse", "ACGT", "ACGT", 1, 10000, (0, 0, 0)),
    ("poly_forward", "AAAA", "TTTT", 0, 10000, (4, 0, 0)),
    ("poly_reverse", "AAAA", "TTTT", 1, 10000, (0, 0, 0)),
    ("reverse_reads_backwards", "AACG", "CGTT", 1, 10000, (0, 0, 0)),
    ("reverse_one_off", "AACG", "CGTA", 1, 10000, (1, 0, 0)),
    ("lower_and_u", "acgu", "ACGT", 0, 10000, (0, 0, 0)),
    ("u_reverse", "AAUU", "aauu", 1, 10000, (0, 0, 0)),
    ("class4_query", "ACNT", "ACGT", 0, 10000, (0, 3, 0)),
    ("class4_subject_last", "ACGT", "ACGR", 0, 10000, (0, 3, 0)),
    ("class4_first", "-CGT", "ACGT", 1, 10000, (0, 3, 0)),
    ("shift_31", "A" * 10, "A" * 41, 0, 10000, (31, 0, 0)),
    ("shift_32", "A" * 10, "A" * 42, 0, 10000, (0, 2, 0)),
    ("shift_minus_31", "C" * 41, "C" * 10, 0, 10000, (31, 0, 0)),
    ("shift_minus_32", "C" * 42, "C" * 10, 0, 10000, (0, 2, 0)),
    ("poly_32", "A" * 32, "C" * 32, 0, 10000, (32, 0, 0)),
    ("poly_33_saturated", "A" * 33, "C" * 33, 0, 10000, (33, 0, 1)),
    ("poly_40_saturated", "A" * 40, "C" * 40, 0, 10000, (40, 0, 1)),
    ("max_seg_exact", "ACGTA", "ACGTA", 0, 5, (0, 0, 0)),
    ("max_seg_plus_one_query", "ACGTAC", "ACGTA", 0, 5, (0, 1, 0)),
    ("max_seg_plus_one_subject", "ACGTA", "ACGTAC", 0, 5, (0, 1, 0)),
    ("length_before_shift_before_n", "N" * 50, "A" * 6, 0, 5, (0, 1, 0)),
    ("shift_before_n", "N" * 50, "A" * 6, 0, 100, (0, 2, 0)),
]

LENGTHS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097]
SHIFTS = [-32, -31, -1, 0, 1, 31, 32]


def _sub(seq, at):
    return seq[:at] + ("C" if seq[at] == "A" else "A") + seq[at + 1:]


def boundary_cases(seed=11):
    """The boundary shapes, forward; every one also turns up once with reverse = 1 (the subject's text reverse-complemented, so
    that the segment spells the same pair)."""
    rng = random.Random(seed)
    out = []
    for n in LENGTHS:
        x = rand_seq(rng, n)
        out.append((f"len{n}_same", x, x, 0, 10000))
        out.append((f"len{n}_sub_first", x, _sub(x, 0), 0, 10000))
        out.append((f"len{n}_sub_last", x, _sub(x, n - 1), 0, 10000))
    for n in (40, 500):
        for d in SHIFTS:
            x = rand_seq(rng, n)
            at = (n + min(d, 0)) // 2
            s = x[:at] + rand_seq(rng, d) + x[at:] if d >= 0 else x[:at] + x[at - d:]
            out.append((f"shift{d}_len{n}", x, s, 0, 10000))
    # a block of b bases more on the subject at one place and b bases more on the query at another: the path has to leave the main
    # diagonal by b.  b = E = 16 stays inside the band and exact; b = 17 is forced to the band's edge
    for b in (16, 17):
        core = [rand_seq(rng, 150) for _ in range(3)]
        blk_s, blk_q = rand_seq(rng, b), rand_seq(rng, b)
        out.append((f"block{b}_start", core[0] + core[1] + blk_q + core[2], blk_s + core[0] + core[1] + core[2], 0, 10000))
        out.append((f"block{b}_end", blk_q + core[0] + core[1] + core[2], core[0] + core[1] + core[2] + blk_s, 0, 10000))
        out.append((f"block{b}_middle", core[0] + blk_q + core[1] + core[2], core[0] + core[1] + blk_s + core[2], 0, 10000))
        out.append((f"block{b}_inserted", core[0] + core[1], core[0] + blk_s + core[1], 0, 10000))
    out.append(("poly_a_poly_c", "A" * 300, "C" * 300, 0, 10000))
    x = rand_seq(rng, 200)
    out.append(("max_seg_exact", x, x[:190], 0, 200))
    out.append(("max_seg_plus_one", x, x[:190], 0, 199))
    out.append(("class4_first", "N" + x[1:], x, 0, 10000))
    out.append(("class4_last", x, x[:-1] + "n", 0, 10000))
    out.append(("lower_case", x.lower(), x, 0, 10000))
    out.append(("u_for_t", x.replace("T", "U"), x.replace("T", "u"), 0, 10000))
    pal = rand_seq(rng, 60)
    out.append(("palindrome", pal + revcomp(pal), pal + revcomp(pal), 1, 10000))
    rev = [(name + "_rev", q, revcomp(s), 1, m) for name, q, s, r, m in out if not r]
    return out + rev


def mutated_pairs(n, seed, max_len=600):
    """Seeded pairs: a random query of 1 .. max_len bases and a copy with substitutions and indel blocks of 1 .. 20 bases."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        lq = rng.randint(1, max_len) if i % 5 else rng.randint(1, 40)
        q = rand_seq(rng, lq)
        s = list(q)
        for _ in range(rng.choice([0, 1, 2, 5, 20])):
            s[rng.randrange(len(s))] = rng.choice("ACGT")
        for _ in range(rng.choice([0, 0, 1, 2, 3])):
            at, b = rng.randrange(len(s) + 1), rng.randint(1, 20)
            if rng.random() < 0.5:
                s[at:at] = list(rand_seq(rng, b))
            elif len(s) > b:
                del s[at:at + b]
        s = "".join(s) or "A"
        rev = i % 3 == 0
        out.append((f"pair{i}", q, revcomp(s) if rev else s, 1 if rev else 0, 10000))
    return out
