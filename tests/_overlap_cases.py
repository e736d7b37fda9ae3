"""The overlap goldens' cases as the tests read them, and the seeded generator of the synthetic set.  Test infrastructure only.

The synthetic set's inputs (contigs and paths) are not committed: they are a pure function of the seed recorded in the
golden's meta, re-made here and checked against the recorded digest; the golden holds what the reference answered."""
import hashlib
import json
import os
import random
import atexit
import shutil
import tempfile

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COMP = str.maketrans("ACGT", "TGCA")
_TMP = None


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def mutate(rng, s, sub, indel):
    out = []
    for c in s:
        x = rng.random()
        if x < sub:
            out.append(rng.choice([b for b in "ACGT" if b != c]))
        elif x < sub + indel:
            if rng.random() < 0.5:
                out.append(c + rng.choice("ACGT"))
        else:
            out.append(c)
    return "".join(out)


def make_synth(seed=20261016, n_paths=40):
    """-> (records [(id, seq)], paths [[(contig, ori, start, end, raw_gap)]])"""
    rng = random.Random(seed)
    records, paths = [], []
    for p in range(n_paths):
        n_nodes = rng.choice([2, 2, 3, 4, 5, 8, 12, 20]) if p else 20
        pieces, gaps = [], []
        prev_tail = None  # the text the next node has to begin with (the overlap, as the next contig holds it)
        for i in range(n_nodes):
            body = rand_seq(rng, rng.choice([40, 120, 300, 500, 800, 1200]))
            piece = (prev_tail or "") + body
            if i + 1 < n_nodes:
                kind = rng.choice(["clean", "clean", "diverged", "diverged", "diverged", "sparse", "sparse", "sparse", "repeat", "islands", "none", "gap", "long", "tiny"])
                if kind == "gap":
                    gaps.append(rng.choice([0, 20, 137]))
                    prev_tail = None
                else:
                    o = {"tiny": rng.choice([1, 2, 5, 14, 15, 24, 25, 26]), "long": rng.randint(2500, 4000)}.get(kind, rng.randint(30, 700))
                    ov = rand_seq(rng, o)
                    if kind == "repeat":
                        unit = rand_seq(rng, rng.randint(18, 60))
                        at = rng.randint(0, len(ov))
                        ov = (ov[:at] + unit * rng.randint(2, 4) + ov[at:])
                    piece += ov
                    other = ov
                    if kind == "diverged":
                        other = mutate(rng, ov, rng.choice([0.01, 0.03, 0.06]), rng.choice([0.0, 0.004, 0.01]))
                    elif kind == "sparse":  # so diverged that single shared minimizers are all there is
                        other = mutate(rng, ov, rng.choice([0.1, 0.14, 0.18]), 0.0)
                    elif kind == "none":
                        other = rand_seq(rng, len(ov))
                    elif kind == "islands":
                        for tgt in (0, 1):
                            t = list(piece if tgt == 0 else other)
                            for _ in range(rng.randint(1, 3)):
                                lo_ok = len(t) - len(ov) - 40 if tgt == 0 else 1
                                at = rng.randint(max(1, lo_ok), len(t) - 2)
                                for q in range(at, min(len(t) - 1, at + rng.choice([1, 3, 17, 40]))):
                                    t[q] = "N"
                            if tgt == 0:
                                piece = "".join(t)
                            else:
                                other = "".join(t)
                    # the raw gap is the scaffolder's estimate: close to the true overlap, sometimes off, sometimes beyond the node
                    est = len(ov) + rng.choice([0, 0, 0, -3, 4, 11, -20, 60])
                    if rng.random() < 0.06:
                        est = len(piece) + rng.randint(1, 300)  # an overlap longer than the segment (l > r)
                    gaps.append(-max(1, est))
                    prev_tail = other
                    if other[0] == "N":
                        prev_tail = "A" + other[1:]
            else:
                gaps.append(rng.choice([0, 0, 20, -50]))  # the last node's raw gap is read by the position filter too
            pieces.append(piece)
        nodes = []
        for i, piece in enumerate(pieces):
            ori = rng.choice("+-")
            fl, fr = rand_seq(rng, rng.choice([0, 0, 7, 33])), rand_seq(rng, rng.choice([0, 0, 16, 50]))
            text = piece if ori == "+" else piece.translate(COMP)[::-1]
            cid = f"p{p}c{i}"
            records.append((cid, fl + text + fr))
            nodes.append((cid, ori, len(fl), len(fl) + len(text), gaps[i]))
        paths.append(nodes)
    return records, paths


def fasta_text(records):
    return "".join(f">{rid}\n{seq}\n" for rid, seq in records)


def paths9(records, paths):
    "the nodes in format_paths' shape (gap_size = the raw gap, at least 20)"
    size = {rid: len(seq) for rid, seq in records}
    return [[[c, o, s, e, size[c], "", "", max(g, 20), g] for c, o, s, e, g in path] for path in paths]


def digest(records, paths):
    return hashlib.sha256((fasta_text(records) + json.dumps(paths)).encode("ascii")).hexdigest()


def load_case(path):
    """-> (golden document with "paths" filled in, path of the case's FASTA file)"""
    with open(path, encoding="ascii") as fh:
        doc = json.load(fh)
    syn = doc["meta"].get("synth")
    if syn is None:
        return doc, os.path.join(GOLDEN, "fasta", doc["meta"]["fasta"])
    records, paths = make_synth(syn["seed"], syn["n_paths"])
    assert digest(records, paths) == syn["sha256"], "the seeded generator no longer gives the inputs the golden was recorded on"
    doc["paths"] = paths9(records, paths)
    global _TMP
    if _TMP is None:  # this process's own directory, removed when it ends
        _TMP = tempfile.mkdtemp(prefix="overlap_synth_")
        atexit.register(shutil.rmtree, _TMP, ignore_errors=True)
    fasta = os.path.join(_TMP, f"{syn['sha256'][:16]}.fa")
    if not os.path.exists(fasta):
        with open(fasta, "w", encoding="ascii") as fh:
            fh.write(fasta_text(records))
    return doc, fasta
