"""The lines of <prefix>.report.tsv (Ntjoin.write_report): one row per file from a report as MxEngine.assembly_report and
MxEngine.scaffold_report return it, and those of <prefix>.assess.tsv and <prefix>.breakpoints.bed (Ntjoin.write_assess) from what
MxEngine.synteny_assess returns, and those of <prefix>.identity.tsv (Ntjoin.write_identity) from what MxEngine.synteny_identity returns.
The numbers are the library's (report.hip, assess.hip, identity.hip); only the text is formed here."""

COLUMNS = ("file records bases A C G T N other lower gaps gap_bases max_gap n n_min sum min max N50 L50 N75 L75 N90 L90 "
           "ctg_n ctg_n_min ctg_sum ctg_min ctg_max ctg_N50 ctg_L50 ctg_N75 ctg_L75 ctg_N90 ctg_L90").split()
_COUNTS = ("n_records", "bases", "a", "c", "g", "t", "n", "other", "lower", "n_gaps", "gap_bases", "max_gap")
_BLOCK = ("n", "n_min", "sum", "min", "max", "n50", "l50", "n75", "l75", "n90", "l90")


def row(name, rep):
    cells = [name] + [rep[k] for k in _COUNTS] + [rep["scaffold"][k] for k in _BLOCK] + [rep["contig"][k] for k in _BLOCK]
    assert len(cells) == len(COLUMNS)
    return "\t".join(str(c) for c in cells)


# ---- <prefix>.assess.tsv and <prefix>.breakpoints.bed (Ntjoin.write_assess): the numbers are the library's (assess.hip) -------------
ASSESS_COLUMNS = ("query reference query_records query_bases reference_bases anchors blocks chains aligned_query_bases "
                  "covered_reference_bases chained_reference_bases NA50 LA50 NGA50 LGA50 NGA75 LGA75 NGA90 LGA90 NG50 LG50 "
                  "translocations_join translocations_contig inversions_join inversions_contig relocations_join relocations_contig").split()
BP_KINDS = ("translocation", "inversion", "relocation")   # by capi.BP_*


def assess_row(query, reference, query_records, anchors, res):
    "one row of <prefix>.assess.tsv from what MxEngine.synteny_assess returns; anchors = the blocks call's n_anchors_total"
    na, nga, ng = res["na"], res["nga"], res["ng"]
    cells = [query, reference, query_records, res["query_bases"], res["subject_bases"], anchors, res["n_blocks"], res["n_chains"],
             res["aligned_query"], res["covered_subject"], res["chained_subject"], na["n50"], na["l50"], nga["n50"], nga["l50"], nga["n75"],
             nga["l75"], nga["n90"], nga["l90"], ng["n50"], ng["l50"]]
    cells += [res["breakpoints"][(kind, j)] for kind in range(3) for j in (1, 0)]
    assert len(cells) == len(ASSESS_COLUMNS)
    return "\t".join(str(c) for c in cells)


def breakpoint_lines(res, query_names, reference, subject_names):
    """the lines of <prefix>.breakpoints.bed for one reference: per breakpoint the query record's name, min(q_lo, q_hi),
    max(q_lo, q_hi, min + 1), <kind>|<join or contig>, the reference assembly's name, and the subject record of the chain on either
    side with its strand"""
    ch, bp = res["chains"], res["bps"]
    side = lambda c: subject_names[int(ch["s_record"][c])] + ("-" if int(ch["reverse"][c]) else "+")  # noqa: E731
    out = []
    for c, kind, j, lo, hi in zip(*[[int(x) for x in bp[name]] for name in ("chain", "kind", "at_join", "q_lo", "q_hi")]):
        start = min(lo, hi)
        cols = (query_names[int(ch["q_record"][c])], start, max(lo, hi, start + 1), BP_KINDS[kind] + "|" + ("join" if j else "contig"), reference,
                side(c), side(c + 1))
        out.append("\t".join(str(x) for x in cols) + "\n")
    return out


# ---- <prefix>.identity.tsv (Ntjoin.write_identity): the numbers are the library's (identity.hip) ------------------------------------
IDENTITY_COLUMNS = ("query reference blocks segments aligned skipped_len skipped_shift skipped_n saturated block_query_bases aligned_query "
                    "aligned_subject edits edits_per_100kbp").split()


def identity_row(query, reference, res):
    """one row of <prefix>.identity.tsv from what MxEngine.synteny_identity returns; edits_per_100kbp = edits * 10^5 / max(aligned_query,
    aligned_subject) in integers, two decimals, floored (0.00 where nothing was aligned)"""
    den = max(res["aligned_q"], res["aligned_s"])
    cents = res["edits"] * 10 ** 7 // den if den else 0
    cells = [query, reference, res["n_blocks"], res["n_segments"], res["n_aligned"], res["n_skip_len"], res["n_skip_shift"], res["n_skip_n"],
             res["n_saturated"], res["block_q"], res["aligned_q"], res["aligned_s"], res["edits"], f"{cents // 100}.{cents % 100:02d}"]
    assert len(cells) == len(IDENTITY_COLUMNS)
    return "\t".join(str(c) for c in cells)
