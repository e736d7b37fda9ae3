"""The assembly report restated in a dozen lines of Python (the contract of include/ntjoin_mx.h under "the assembly report"): what
mxg_assembly_report, mxg_scaffold_report and tools/seqstat_check.cpp must reproduce.  No program for this exists on the machines the
suite runs on (QUAST and abyss-fac are absent), so this restatement is the oracle."""
import re

COLUMNS = ("file records bases A C G T N other lower gaps gap_bases max_gap n n_min sum min max N50 L50 N75 L75 N90 L90 "
           "ctg_n ctg_n_min ctg_sum ctg_min ctg_max ctg_N50 ctg_L50 ctg_N75 ctg_L75 ctg_N90 ctg_L90").split()
BLOCK = ("n", "n_min", "sum", "min", "max", "n50", "l50", "n75", "l75", "n90", "l90")


def records(text):
    "the bases of every record of FASTA bytes: header lines begin with '>' at the start of a line"
    out = []
    for line in text.split(b"\n"):
        if line.startswith(b">"):
            out.append([])
        elif out:
            out[-1].append(line.replace(b"\r", b""))
    return [b"".join(parts) for parts in out]


def contiguity(lengths, min_len):
    sel = sorted((x for x in lengths if x >= min_len), reverse=True)
    block = dict.fromkeys(BLOCK, 0)
    block["n"] = len(lengths)
    if not sel:
        return block
    block.update(n_min=len(sel), sum=sum(sel), min=sel[-1], max=sel[0])
    for x in (50, 75, 90):
        run = 0
        for j, length in enumerate(sel, 1):
            run += length
            if 100 * run >= x * block["sum"]:
                block[f"n{x}"], block[f"l{x}"] = length, j
                break
    return block


def report(text, min_gap=10, min_len=500):
    recs = records(text)
    gaps, contigs = [], []
    for seq in recs:
        at = 0
        for m in re.finditer(b"[Nn]+", seq):
            if m.end() - m.start() >= min_gap:
                gaps.append(m.end() - m.start())
                contigs.append(m.start() - at)
                at = m.end()
        contigs.append(len(seq) - at)
    contigs = [c for c in contigs if c]
    everything = b"".join(recs)
    count = lambda letters: sum(everything.count(bytes([c])) for c in letters)  # noqa: E731
    rep = {"n_records": len(recs), "bases": len(everything), "a": count(b"Aa"), "c": count(b"Cc"), "g": count(b"Gg"), "t": count(b"TtUu"),
           "n": count(b"Nn"), "lower": sum(1 for c in everything if 97 <= c <= 122),
           "n_gaps": len(gaps), "gap_bases": sum(gaps), "max_gap": max(gaps, default=0),
           "scaffold": contiguity([len(s) for s in recs], min_len), "contig": contiguity(contigs, min_len),
           "gap_len": sorted(gaps), "contig_len": sorted(contigs), "min_gap": min_gap, "min_len": min_len}
    rep["other"] = rep["bases"] - rep["a"] - rep["c"] - rep["g"] - rep["t"] - rep["n"]
    return rep


def normal(rep):
    "a report of the engine (numpy lists in any order) in the restatement's form"
    out = dict(rep)
    out["gap_len"] = sorted(int(x) for x in rep["gap_len"])
    out["contig_len"] = sorted(int(x) for x in rep["contig_len"])
    return out


def tsv_row(name, rep):
    "the row of <prefix>.report.tsv"
    sc, ct = rep["scaffold"], rep["contig"]
    cells = [name] + [rep[k] for k in ("n_records", "bases", "a", "c", "g", "t", "n", "other", "lower", "n_gaps", "gap_bases", "max_gap")]
    cells += [sc[k] for k in BLOCK] + [ct[k] for k in BLOCK]
    return "\t".join(str(c) for c in cells)
