"""CPU tests of the many-records cases (tests/_many_records.py) that tests/test_gpu_many_records.py feeds the device: every case through
both restatements (tests/_synteny_restatement.py, tests/_assess_restatement.py) with the conditions that give the device tests their
teeth asserted here, so that a case that stops meeting them fails without a GPU first; a model of the device's rule for the union of
subject intervals whose sort reads too few key bits, which must DIFFER from the restatement from 257 and from 65 537 subject records
on (the role tests/test_maxscan_model_cpu.py plays for the running maximum); and the same block and anchor lists through
tools/assess_check.cpp and tools/synteny_check.cpp, built plainly and with AddressSanitizer + UndefinedBehaviorSanitizer linked into
the stand-alone program (the fixtures of tests/test_assess_cpu.py and tests/test_synteny_cpu.py; nothing is preloaded).

The record counts are those of _many_records.COUNTS; a sort of eight passes takes 2^24 records and is not built (see there)."""
import functools
import subprocess

import pytest

from tests import _assess_cases as AC, _assess_restatement as A, _many_records as MR, _synteny_cases as cases, _synteny_restatement as R
from tests.test_assess_cpu import _check as assess_check, _input_text as assess_input, exe as assess_exe   # noqa: F401  (a fixture)
from tests.test_synteny_cpu import _check as synteny_check, _input_text as synteny_input, exe as synteny_exe   # noqa: F401  (a fixture)

ZEROS = dict(n50=0, l50=0, n75=0, l75=0, n90=0, l90=0)


@functools.lru_cache(maxsize=None)
def restated(builder, arg, table=None, lengths=None, min_anchors=2):
    "-> (the case, its blocks by the synteny restatement, their assessment by the assess restatement), computed once"
    case = MR.cached(builder, arg)
    if table:
        pieces, first = MR.TABLES[table](case)
        case = dict(case, pieces=pieces, first=first)
    if lengths:
        case = dict(case, lengths=case[lengths])
    case = dict(case, min_anchors=min_anchors)
    vpos, vrec = cases.graph_arrays(case)
    syn = R.synteny(vpos, vrec, case["q"], case["s"], case["k"], case["max_gap"], case["min_anchors"], case["min_span"], case["pieces"], case["first"])
    got = A.assess(syn["blocks"], case["k"], R.query_lengths(case["lengths"][case["q"]], case["pieces"], case["first"]), case["lengths"][case["s"]],
                   pieces=case["pieces"], first=case["first"], **case["assess"])
    return case, syn, got


def as_block_case(case, syn):
    "what tools/assess_check reads: the kept blocks, the lengths the assessment saw, the table"
    return AC.block_case(syn["blocks"], R.query_lengths(case["lengths"][case["q"]], case["pieces"], case["first"]), case["lengths"][case["s"]],
                         case["pieces"], case["first"], k=case["k"], **case["assess"])


# ---- 1: subject records -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_s", MR.COUNTS)
def test_subject_cases(n_s):
    case, syn, got = restated("many_subject_case", n_s, lengths="nx_lengths")
    n = MR.subject_blocks(n_s)
    recs = got["chains"]["s_record"]
    assert len(case["asms"][0]) == n_s and len(case["asms"][1]) == 1
    assert len(syn["blocks"]) == got["n_chains"] == n and syn["n_anchors_total"] == 2 * n
    assert set(recs) == set(range(n_s))   # every subject record is in use
    for r in MR.MARKS + (n_s - 1,):
        assert r >= n_s or recs.count(r) >= 3
    if n_s > 1:
        assert recs != sorted(recs) and recs != sorted(recs, reverse=True)
    assert got["covered_subject"] < got["chained_subject"] == 82 * n
    assert sum(got["chains"]["reverse"]) == n // 5
    # all three Nx blocks are comparisons of non-zero figures
    assert got["na"]["l50"] == n and got["nga"]["l50"] > 0 and got["ng"]["l50"] == 1 and got["na"]["n50"] == got["nga"]["n50"] == 82
    # the breakpoints: one at every chain border; from 127 records on nearly all of them are translocations off a join
    assert got["n_breakpoints"] == n - 1 and all(got["breakpoints"][(kind, 1)] == 0 for kind in range(3))
    if n_s >= 127:
        assert got["breakpoints"][(A.TRANSLOCATION, 0)] > 0.98 * n


@pytest.mark.parametrize("n_s", MR.COUNTS)
def test_a_sort_of_too_few_key_bits_gives_another_union(n_s):
    """the device's rule (stable sort by the key's low bits, running maximum, as_uncovered) equals the restatement at the full key
    width, and differs from it once a record number no longer fits the bits the sort reads: 40 bits (five passes) hold records up
    to 255, 48 bits (six passes) records up to 65 535.  So a pass too few, or a result read from the wrong buffer, shows in
    covered_subject of these cases"""
    _case, _syn, got = restated("many_subject_case", n_s, lengths="nx_lengths")
    chains = list(zip(got["chains"]["s_record"], got["chains"]["s_start"], got["chains"]["s_end"]))
    want = got["covered_subject"]
    assert MR.cover_by_truncated_sort(chains, 64) == want
    bits = 32 + n_s.bit_length()   # what assess.hip asks for: 32 + bits_of(n_subject_records)
    assert MR.cover_by_truncated_sort(chains, bits) == want and MR.cover_by_truncated_sort(chains, 8 * ((bits + 7) // 8)) == want
    assert (MR.cover_by_truncated_sort(chains, 40) != want) == (n_s >= 257)
    assert (MR.cover_by_truncated_sort(chains, 48) != want) == (n_s >= 65537)
    # the number of passes on either side of each count: 5 | 6 | 7
    assert (bits + 7) // 8 == (5 if n_s <= 255 else 6 if n_s <= 65535 else 7)


@pytest.mark.parametrize("n_s", [256, 65537])
def test_two_record_subject_on_the_same_handle(n_s):
    "the third assembly of with_two_record_subject keeps every vertex and gives the same number of blocks on a subject of two records"
    case = MR.with_two_record_subject(MR.cached("many_subject_case", n_s))
    vpos, vrec = cases.graph_arrays(case)
    assert len(vpos) == 3 and len(vpos[2]) == 2 * MR.subject_blocks(n_s) and set(vrec[2]) == {0, 1}
    kept = R.synteny(vpos, vrec, 1, 2, case["k"], case["max_gap"], 2, 0)["blocks"]
    assert len(kept) == MR.subject_blocks(n_s) and {b[4] for b in kept} == {0, 1}


# ---- 2: query records -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_q", MR.QUERY_COUNTS)
def test_query_cases(n_q):
    case, syn, got = restated("many_query_case", n_q)
    assert len(case["asms"][1]) == n_q and len(case["asms"][0]) == 3
    assert len(syn["blocks"]) == got["n_chains"] == n_q and got["n_breakpoints"] == 0
    assert got["chains"]["q_record"] == list(range(n_q)) and got["chains"]["s_record"] == [b % 3 for b in range(n_q)]
    assert len(set(case["lengths"][1])) >= 40
    assert all(b[3] <= case["lengths"][1][b[1]] and b[6] <= case["lengths"][0][b[4]] for b in syn["blocks"])   # the lengths are true
    assert got["na"]["l50"] > 0 and got["nga"]["l50"] > 0 and got["ng"]["l50"] > 0 and got["ng"]["l90"] > got["ng"]["l50"]
    assert got["ng"]["n50"] != got["ng"]["n90"]


@pytest.mark.parametrize("n_q", [1025, 65537])
def test_few_chains_cases(n_q):
    case, syn, got = restated("few_chains_case", n_q)
    assert len(case["asms"][1]) == n_q and sum(1 for _rid, mxs in case["asms"][1] if mxs) == 3
    assert len(syn["blocks"]) == 6 and got["n_chains"] == 3 and got["chains"]["q_record"] == [0, n_q // 2, n_q - 1]
    assert got["ng"]["l50"] > n_q // 4 and got["ng"]["l90"] > got["ng"]["l50"] and len(set(case["lengths"][1])) >= 40
    _, none, zero = restated("few_chains_case", n_q, min_anchors=3)
    assert none["blocks"] == [] and none["n_anchors_total"] == 12
    assert zero["n_chains"] == zero["aligned_query"] == zero["chained_subject"] == zero["covered_subject"] == 0
    assert zero["na"] == zero["nga"] == ZEROS and zero["ng"] == got["ng"]


@pytest.mark.parametrize("name", sorted(MR.TABLES))
def test_piece_tables_over_65537_source_records(name):
    case, syn, got = restated("many_query_case", 65537, table=name)
    pieces, first = case["pieces"], case["first"]
    used = [p[0] for p in pieces if p[3] != MR.GAP]
    if name == "high_falling":
        assert used == list(range(65536, 255, -1)) and len(syn["blocks"]) == got["n_chains"] == 65537 - 256
    else:
        assert used == list(range(65537)) and len(syn["blocks"]) == got["n_chains"] == 65537
        assert sum(p[3] == MR.REV for p in pieces) == 65536 // 2
    joins = sum(got["breakpoints"][(kind, 1)] for kind in range(3))
    if name == "dealt":
        sizes = {(b - a + 1) // 2 for a, b in zip(first, first[1:])}
        assert sizes == set(range(1, 41)) and any(p[3] == MR.GAP for p in pieces)
        assert joins == got["n_breakpoints"] == 65537 - (len(first) - 1) and got["breakpoints"][(A.TRANSLOCATION, 1)] > 60000
    else:
        assert got["n_breakpoints"] == 0 and len(first) - 1 == len(pieces)
    assert got["ng"]["l50"] > 0 and got["na"]["l50"] > 0


# ---- 3: PAF ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["many_subject_case", "many_query_case"])
def test_paf_cases(builder):
    case = MR.cached(builder, 65537)
    syn = restated(builder, 65537, None, "nx_lengths" if "nx_lengths" in case else None)[1]
    paf = MR.paf_case(case)
    vpos, vrec = cases.graph_arrays(paf)
    through = R.synteny(vpos, vrec, 1, 0, paf["k"], paf["max_gap"], 2, 0, paf["pieces"], paf["first"])
    assert through["blocks"] == syn["blocks"]   # (a table of whole FWD pieces changes nothing)
    names = paf["names"]
    assert {len(x) for x in names} == (set(range(1, 41)) if len(names) > 40 else {len(names[0])}) and len(names) == len(case["asms"][1])
    text = R.paf(syn["blocks"], names, R.query_lengths(paf["lengths"][1], paf["pieces"], paf["first"]), [rid for rid, _ in paf["asms"][0]],
                 paf["lengths"][0], paf["k"])
    assert text.count("\n") == len(syn["blocks"]) >= 65537 and len(text) > 3_000_000
    if builder == "many_subject_case":
        assert "\trec65536\t" in text and "\trec0\t" in text


# ---- the device route's code on the host: tools/assess_check, tools/synteny_check --------------------------------------------------
SMALL = [("many_subject_case", n, None, "nx_lengths") for n in MR.COUNTS if n <= 257] + \
        [("many_query_case", n, None, None) for n in MR.QUERY_COUNTS if n <= 1025] + [("few_chains_case", 1025, None, None)]
LARGE = [("many_subject_case", n, None, "nx_lengths") for n in MR.COUNTS if n > 257] + \
        [("many_query_case", n, None, None) for n in MR.QUERY_COUNTS if n > 1025] + [("few_chains_case", 65537, None, None)] + \
        [("many_query_case", 65537, name, None) for name in sorted(MR.TABLES)]


@functools.lru_cache(maxsize=None)
def tool_inputs(builder, arg, table=None, lengths=None, min_anchors=2):
    "-> (what tools/assess_check reads, what tools/synteny_check reads) of a case, written once for the plain and the sanitized program"
    case, syn, _got = restated(builder, arg, table, lengths, min_anchors)
    return assess_input(as_block_case(case, syn)), synteny_input(case)


def run_tool(exe, text, tmp_path):
    f = tmp_path / "case.txt"
    f.write_text(text)
    res = subprocess.run([exe, str(f)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    return [line.split() for line in res.stdout.splitlines()]


def assess_tool_agrees(exe, tmp_path, *key):
    "every line tools/assess_check prints against the restatement (the comparison of tests/test_assess_cpu.py, the restatement computed once)"
    want = restated(*key)[2]
    lines = run_tool(exe, tool_inputs(*key)[0], tmp_path)
    assert [int(x) for x in lines[0]] == [want["n_blocks"], want["n_chains"], want["n_breakpoints"]] + \
        [want["breakpoints"][(kind, j)] for kind in range(3) for j in range(2)] + \
        [want[name] for name in ("query_bases", "subject_bases", "aligned_query", "chained_subject", "covered_subject")]
    assert lines[1][0] == "X" and [int(x) for x in lines[1][1:]] == [want[b][f"{c}{x}"] for b in ("na", "nga", "ng") for x in (50, 75, 90) for c in "nl"]
    assert [[int(x) for x in v[1:]] for v in lines[2:] if v[0] == "C"] == [list(row) for row in zip(*[want["chains"][name] for name in A.CHAIN_FIELDS])]
    assert [[int(x) for x in v[1:]] for v in lines[2:] if v[0] == "B"] == [list(row) for row in zip(*[want["bps"][name] for name in A.BP_FIELDS])]
    assert len(lines) == 2 + want["n_chains"] + want["n_breakpoints"]


def synteny_tool_agrees(exe, tmp_path, *key):
    "every line tools/synteny_check prints against the restatement"
    want = restated(*key)[1]
    lines = [[int(x) for x in v] for v in run_tool(exe, tool_inputs(*key)[1], tmp_path)]
    assert lines[0] == [want["n_anchors_total"], want["n_links"]] and [tuple(v[:8]) for v in lines[1:]] == want["blocks"]
    assert all(v[8] == min(v[0] * MR.K, v[3] - v[2], v[6] - v[5]) and v[9] == max(v[3] - v[2], v[6] - v[5]) for v in lines[1:])


def test_assess_check_on_the_small_counts(assess_exe, tmp_path):   # noqa: F811
    case, syn, got = restated(*SMALL[5])
    assert assess_check(assess_exe, as_block_case(case, syn), tmp_path) == got   # (the comparison of the tool's own tests, once)
    for key in SMALL:
        assess_tool_agrees(assess_exe, tmp_path, *key)


@pytest.mark.parametrize("key", LARGE, ids=lambda key: "-".join(str(x) for x in key[:3] if x))
def test_assess_check_past_65535_records(assess_exe, key, tmp_path):   # noqa: F811
    assess_tool_agrees(assess_exe, tmp_path, *key)


def test_assess_check_without_blocks(assess_exe, tmp_path):   # noqa: F811
    assess_tool_agrees(assess_exe, tmp_path, "few_chains_case", 65537, None, None, 3)
    assert restated("few_chains_case", 65537, None, None, 3)[2]["ng"] != ZEROS


def test_synteny_check_on_the_small_counts(synteny_exe, tmp_path):   # noqa: F811
    synteny_check(synteny_exe, restated(*SMALL[5])[0], tmp_path)   # (the comparison of the tool's own tests, once)
    for key in SMALL:
        synteny_tool_agrees(synteny_exe, tmp_path, *key)


@pytest.mark.parametrize("key", LARGE, ids=lambda key: "-".join(str(x) for x in key[:3] if x))
def test_synteny_check_past_65535_records(synteny_exe, key, tmp_path):   # noqa: F811
    synteny_tool_agrees(synteny_exe, tmp_path, *key)


# ---- 4: the FASTA files of the identity tests ------------------------------------------------------------------------------------------
def test_short_contig_files(tmp_path):
    """300 contigs of 200 to 900 bases: every 4096-byte tile of the target holds bytes of several records, and at least 250 of its
    256-byte sub-tiles (the unit text_of_base clamps its scan in, ntjoin_amd/csrc/text_index.h) do, with at least 250 sub-tile
    borders inside a record.  A file of 150 kbp has fewer than 40 tiles of 4096 bytes, so no count of 250 can be theirs"""
    from tests import _identity_restatement as IR
    files = MR.short_contig_files(tmp_path)
    again = MR.short_contig_files(tmp_path)
    assert again["ttexts"] == files["ttexts"] and again["rtexts"] == files["rtexts"]
    contigs = files["contigs"]
    assert len(contigs) == 300 and min(map(len, contigs)) == 200 and max(map(len, contigs)) == 900
    assert [len(IR.bases(t)) for t in files["ttexts"]] == [len(c) for c in contigs] and 140000 < sum(map(len, contigs)) < 160000
    assert len(files["rtexts"]) == 3 and 140000 < sum(len(IR.bases(t)) for t in files["rtexts"]) < 160000
    assert contigs[MR.N_RUN].count("N") == 25 and "N" not in contigs[MR.N_RUN][:60] + contigs[MR.N_RUN][-60:]
    assert contigs[MR.LOWER].islower() and sum(c.islower() for c in contigs) == 1
    assert files["ttexts"][MR.ONE_LINE].count("\n") == 1 and len(contigs[MR.ONE_LINE]) > 60
    assert files["ttexts"][MR.CRLF].count("\r\n") == files["ttexts"][MR.CRLF].count("\n") > 3 and sum("\r" in t for t in files["ttexts"]) == 1
    assert all(t.index("\n") == 60 for c, t in enumerate(files["ttexts"]) if c not in (MR.ONE_LINE, MR.CRLF))
    data = open(files["tgt"], "rb").read()
    assert data.count(b">") == 300
    inside, shared, tiles = MR.tile_counts(data, MR.TILE)
    assert shared == tiles >= 35 and inside >= 30
    inside, shared, _ = MR.tile_counts(data, MR.SUB_TILE)
    assert inside >= 250 and shared >= 250
