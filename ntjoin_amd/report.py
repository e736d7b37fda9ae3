"""The lines of <prefix>.report.tsv (Ntjoin.write_report): one row per file from a report as MxEngine.assembly_report and
MxEngine.scaffold_report return it.  The numbers are the library's (report.hip); only the text is formed here."""

COLUMNS = ("file records bases A C G T N other lower gaps gap_bases max_gap n n_min sum min max N50 L50 N75 L75 N90 L90 "
           "ctg_n ctg_n_min ctg_sum ctg_min ctg_max ctg_N50 ctg_L50 ctg_N75 ctg_L75 ctg_N90 ctg_L90").split()
_COUNTS = ("n_records", "bases", "a", "c", "g", "t", "n", "other", "lower", "n_gaps", "gap_bases", "max_gap")
_BLOCK = ("n", "n_min", "sum", "min", "max", "n50", "l50", "n75", "l75", "n90", "l90")


def row(name, rep):
    cells = [name] + [rep[k] for k in _COUNTS] + [rep["scaffold"][k] for k in _BLOCK] + [rep["contig"][k] for k in _BLOCK]
    assert len(cells) == len(COLUMNS)
    return "\t".join(str(c) for c in cells)
