"""GPU tests of the scaffold stage (mxg_write_scaffolds, csrc/scaffold.hip; reference print_scaffolds and print_unassigned,
bin/ntjoin_assemble.py:580-658): the goldens (the reference's own output) end to end through Ntjoin, the generated families of
tests/golden/scaffolds/families against the reference's recorded answers, seeded fuzz and one large call against the restatement (tests/_scaffold_restatement.py), both text layouts, small output windows, the assigned file into a FIFO, and every refusal.  Text only:
every comparison is byte for byte."""
import argparse
import glob
import hashlib
import os
import time

import numpy as np
import pytest

from ntjoin_amd import synth
from ntjoin_amd.engine import MxEngine, MxError
from ntjoin_amd.ntjoin import Ntjoin
from tests import _fifo, _oracle, _scaffold_cases as cases, _scaffold_pin as pin, _scaffold_restatement as rs

pytestmark = pytest.mark.gpu

CASES = sorted(glob.glob(os.path.join(cases.GOLDEN, "scaffolds", "*.json")))
IDS = [os.path.basename(c)[:-5] for c in CASES]
EXPECTED = os.path.join(cases.GOLDEN, "scaffolds", "expected_f-f")
EINVAL, ELIMIT = -1, -5


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


def kept_nodes(paths):
    "paths of format_path's nodes as print_scaffolds keeps them: no '?' node, no path of fewer than two nodes, the last gap zeroed"
    out = []
    for path in paths:
        nodes = [list(nd) for nd in path if nd[1] != "?"]
        if len(nodes) >= 2:
            nodes[-1][7] = 0
            out.append(nodes)
    return out


def run(eng, a, records, paths, out, overlap_gap=None, fold=False):
    "one call of the library -> (assigned, unassigned FASTA, BED as bytes, result dict)"
    index = {rid: r for r, (rid, _) in enumerate(records)}
    rows, first = cases.rows_of(paths, index)
    names = [str(out) + s for s in (".assigned.fa", ".unassigned.fa", ".bed")]
    res = eng.write_scaffolds(a, rows, first, overlap_gap=overlap_gap, fold_case=fold, assigned=names[0], unassigned=names[1], bed=names[2])
    return read(names[0]), read(names[1]), read(names[2]), res


def check_against_restatement(eng, a, records, paths, out, overlap_gap=None, fold=False):
    got = run(eng, a, records, paths, out, overlap_gap, fold)
    text, leads, tails = rs.scaffolds(paths, dict(records), overlap_gap, fold)
    bed, un_fa, n = rs.unassigned(records, paths)
    assert got[0] == text.encode("ascii")
    assert got[1] == un_fa.encode("ascii")
    assert got[2] == bed.encode("ascii")
    assert got[3]["lead_strip"].tolist() == leads and got[3]["tail_strip"].tolist() == tails and got[3]["n_unassigned"] == n
    # the strips of the unassigned intervals (mxg_scaffold_strips), per line of the BED
    seqs, want = dict(records), []
    for line in bed.splitlines():
        rid, lo, hi = line.split("\t")
        text = seqs[rid][int(lo):int(hi)]
        lead = len(text) - len(text.lstrip("Nn"))
        want.append((lead, 0 if lead == len(text) else len(text) - len(text.rstrip("Nn"))))
    lead_u, tail_u = eng.scaffold_strips()
    assert list(zip(lead_u.tolist(), tail_u.tolist())) == want
    return got


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_goldens_end_to_end_through_ntjoin(case, tmp_path, monkeypatch):
    "FASTA -> find_paths -> format_paths -> trim_overlaps -> print_scaffolds: the five files, against the reference's own"
    doc, fasta = cases.load_golden(case)
    name = doc["meta"]["fasta"]
    monkeypatch.chdir(tmp_path)  # the reference's .path names the FASTA as it was given: relative names, as its tests run it
    os.symlink(fasta, name)
    os.symlink(os.path.join(cases.GOLDEN, "fasta", "ref.fa"), "ref.fa")
    n = doc["meta"]["n"]
    args = argparse.Namespace(k=32, FILES=["ref.fa.k32.w1000.tsv"], s=name + ".k32.w1000.tsv", l=1.0, p="out", n=n, overlap_k=15, overlap_w=10)
    nj = Ntjoin(args, fasta={args.FILES[0]: "ref.fa", args.s: name}, w=1000)
    try:
        nj.weights_list = [2.0]
        nj.load_minimizers_scaffold()
        nj.make_minimizer_graph()
        nj.find_paths()
        paths = nj.format_paths()
        assert kept_nodes(paths) == kept_nodes(doc["paths"])  # (the overlap goldens hold the paths as print_scaffolds keeps them)
        adjust = nj.trim_overlaps(paths) if doc["meta"]["overlap"] else None
        if adjust is not None:
            assert [[list(c) for c in a] for a in adjust if a] == doc["adjust"]
        files = nj.print_scaffolds(paths, adjust, n=n, agp=True, overlap_gap=doc["meta"]["overlap_gap"])
        assert files["assigned"] == f"{name}.k32.w1000.n{n}.assigned.scaffolds.fa" and files["bed"] == f"out.{name}.k32.w1000.tsv.unassigned.bed"
        assert read(files["assigned"]) == doc["assigned"].encode("ascii")
        assert read(files["path"]) == doc["path"].encode("ascii")
        records = _oracle.read_fasta(fasta)
        bed, un_fa, _ = rs.unassigned(records, cases.golden_nodes(doc))
        assert read(files["unassigned"]) == un_fa.encode("ascii") and read(files["bed"]) == bed.encode("ascii")
        agp = read(files["agp"]).decode("ascii").splitlines()
        if os.path.basename(case) == "f-f.json":
            for kind, f in (("assigned", "scaf.f-f.fa.k32.w1000.n1.assigned.scaffolds.fa"), ("unassigned", "scaf.f-f.fa.k32.w1000.n1.unassigned.scaffolds.fa"),
                            ("path", "f-f_test.path"), ("bed", "f-f_test.scaf.f-f.fa.k32.w1000.tsv.unassigned.bed")):
                assert read(files[kind]) == read(os.path.join(EXPECTED, f)), kind
        if os.path.basename(case) == "f-f.termN.unassigned.json":  # the lines the reference's own AGP test expects
            assert agp == ["ntJoin0\t1\t1981\t1\tW\t1_f\t5\t1985\t+", "ntJoin0\t1982\t2001\t2\tN\t20\tscaffold\tyes\talign_genus",
                           "ntJoin0\t2002\t4330\t3\tW\t2_f\t1\t2329\t+", "unassigned:0-14\t1\t8\t1\tW\tunassigned\t3\t10\t+"]
        if os.path.basename(case) == "f-r.overlapping.json":
            assert agp == ["ntJoin0\t1\t2033\t1\tW\t1\t1\t2033\t+", "ntJoin0\t2034\t2053\t2\tN\t20\tscaffold\tyes\talign_genus",
                           "ntJoin0\t2054\t4350\t3\tW\t2\t1\t2297\t-"]
    finally:
        nj.close()


@pytest.mark.parametrize("seed", cases.FUZZ_SEEDS)
def test_fuzz_against_restatement(seed, tmp_path):
    "(what the seeds cover and how little they leave out: tests/test_scaffolds_cpu.py)"
    case = cases.fuzz_case(seed)
    fasta = str(tmp_path / "t.fa")
    cases.write_fasta(fasta, case["records"], case["width"], case["final_newline"])
    with MxEngine(k=15, w=10) as eng:
        a = eng.add_fasta("t", 1.0, fasta) if seed % 5 else eng.add_records("t", 1.0, case["records"])
        check_against_restatement(eng, a, case["records"], case["paths"], tmp_path / "o", case["overlap_gap"], case["fold"])
        check_against_restatement(eng, a, case["records"], case["paths"], tmp_path / "p", case["overlap_gap"], not case["fold"])


@pytest.mark.parametrize("seed", [3, 8, 14, 21])
def test_both_text_layouts_give_identical_files(seed, tmp_path, monkeypatch):
    "the file's text in HBM with its tile index (device ingest) and the host parser's text uploaded on first use (MXG_HOST_INGEST=1)"
    case = cases.fuzz_case(seed)
    fasta = str(tmp_path / "t.fa")
    cases.write_fasta(fasta, case["records"], case["width"], case["final_newline"])
    got = []
    for host in (False, True):
        if host:
            monkeypatch.setenv("MXG_HOST_INGEST", "1")
        else:
            monkeypatch.delenv("MXG_HOST_INGEST", raising=False)
        with MxEngine(k=15, w=10) as eng:
            a = eng.add_fasta("t", 1.0, fasta)
            got.append(check_against_restatement(eng, a, case["records"], case["paths"], tmp_path / f"o{int(host)}", case["overlap_gap"], case["fold"])[:3])
            assert ("MXG_HOST_INGEST=1" in eng.knobs()) == host
    assert got[0] == got[1]


def test_small_windows_equal_the_default(tmp_path, monkeypatch):
    "MXG_SCAF_WIN: bytes of output per device window; one emit tile per window makes every file many windows"
    case = cases.fuzz_case(13)
    fasta = str(tmp_path / "t.fa")
    cases.write_fasta(fasta, case["records"], 60)
    got = []
    for win in (None, "8192", "1", "40000"):
        if win is None:
            monkeypatch.delenv("MXG_SCAF_WIN", raising=False)
        else:
            monkeypatch.setenv("MXG_SCAF_WIN", win)
        with MxEngine(k=15, w=10) as eng:
            a = eng.add_fasta("t", 1.0, fasta)
            got.append(check_against_restatement(eng, a, case["records"], case["paths"], tmp_path / f"o{win}", case["overlap_gap"], case["fold"])[:3])
            assert win is None or f"MXG_SCAF_WIN={win}" in eng.knobs()
    assert len(got[0][0]) > 5 * 8192 and len(got[0][1]) > 8192  # several windows of either FASTA
    assert got[1:] == [got[0]] * 3


def test_a_fifo_takes_the_windows_in_order(tmp_path, monkeypatch):
    """the assigned FASTA into a FIFO (no offsets: the windows are written in order at the descriptor's own position), one emit tile
    per window: the bytes of the same call into a regular file.  The fuzz case with the smallest assigned file of three windows."""
    case = cases.fuzz_case(46)
    fasta = str(tmp_path / "t.fa")
    cases.write_fasta(fasta, case["records"], case["width"], case["final_newline"])
    index = {rid: r for r, (rid, _) in enumerate(case["records"])}
    rows, first = cases.rows_of(case["paths"], index)
    monkeypatch.setenv("MXG_SCAF_WIN", str(cases.TILE))
    with MxEngine(k=15, w=10) as eng:
        a = eng.add_fasta("t", 1.0, fasta)
        want = check_against_restatement(eng, a, case["records"], case["paths"], tmp_path / "o", case["overlap_gap"], case["fold"])
        assert f"MXG_SCAF_WIN={cases.TILE}" in eng.knobs() and len(want[0]) > 2 * cases.TILE  # three windows
        names = [str(tmp_path / f) for f in ("f.assigned.fa", "f.unassigned.fa", "f.bed")]
        with _fifo.fifo_reader(names[0], len(want[0])) as drain:
            res = eng.write_scaffolds(a, rows, first, overlap_gap=case["overlap_gap"], fold_case=case["fold"], assigned=names[0],
                                      unassigned=names[1], bed=names[2])
            assert drain() == want[0]
        assert (read(names[1]), read(names[2])) == want[1:3]
        assert res["lead_strip"].tolist() == want[3]["lead_strip"].tolist() and res["n_unassigned"] == want[3]["n_unassigned"]


def test_refusals_write_nothing(tmp_path):
    "every MXG_EINVAL / MXG_ELIMIT of the contract: its code, its message, and no file"
    records = [("a", "NNACGTACGTNN"), ("b", "ACGTACGTAC"), ("n", "NNNNnnNN")]
    fasta = str(tmp_path / "t.fa")
    cases.write_fasta(fasta, records, 5)
    tsv = str(tmp_path / "t.fa.k4.w2.tsv")
    _oracle.load().fasta_to_tsv(fasta, tsv, 4, 2)
    good = [(0, 0, 12, 5, 0, 0, 0), (1, 0, 10, 0, 0, 0, 1)]
    names = [str(tmp_path / f) for f in ("x.fa", "x.un.fa", "x.bed")]

    def fails(eng, asm, code, match, rows, pf, gap=None):
        with pytest.raises(MxError, match=match) as ei:
            eng.write_scaffolds(asm, rows, pf, overlap_gap=gap, assigned=names[0], unassigned=names[1], bed=names[2])
        assert ei.value.code == code
        assert not any(os.path.exists(f) for f in names)

    import torch
    codes = synth.make_reference(1, 4000)[0]
    words, rec_start, rec_len = synth.pack_records([codes])
    d_words = torch.from_numpy(words.view(np.int32)).cuda()
    with MxEngine(k=4, w=2) as eng:
        a = eng.add_fasta("t", 1.0, fasta)
        h = eng.add_records("h", 1.0, records)
        t = eng.add_tsv("tsv", 1.0, tsv)
        pk = eng.add_packed_device("p", 1.0, d_words.data_ptr(), rec_start, rec_len, ids=["g"], keepalive=d_words)
        mz = eng.add_minimizers("m", 1.0, [5, 9], [0, 3], [0, 0], ["a"])
        for asm in (a, h):
            fails(eng, asm, EINVAL, r"\[4, 4\) is not a segment", [good[0], (1, 4, 4, 0, 0, 0, 0)], [0, 2])
            fails(eng, asm, EINVAL, r"\[0, 11\) is not a segment", [good[0], (1, 0, 11, 0, 0, 0, 0)], [0, 2])
            fails(eng, asm, EINVAL, "no record 7", [good[0], (7, 0, 1, 0, 0, 0, 0)], [0, 2])
            fails(eng, asm, EINVAL, "path 1 has 1 node", good + [good[0]], [0, 2, 3])
            fails(eng, asm, EINVAL, "end_adjust 13", [(0, 0, 12, 5, 0, 13, 0), good[1]], [0, 2], gap=20)
            fails(eng, asm, EINVAL, "first piece.*no text left", [(0, 0, 12, 5, 7, 7, 0), good[1]], [0, 2], gap=20)
            fails(eng, asm, EINVAL, "last piece.*no text left", [good[0], (1, 0, 10, 0, 9, 3, 0)], [0, 2], gap=20)
            fails(eng, asm, EINVAL, "first piece is N throughout", [(2, 0, 8, 3, 0, 0, 0), good[1]], [0, 2])
            fails(eng, asm, EINVAL, "first piece is N throughout", [(0, 0, 2, 3, 0, 0, 1), good[1]], [0, 2])
            fails(eng, asm, EINVAL, "last piece is N throughout", [good[0], (0, 10, 12, 0, 0, 0, 0)], [0, 2])
            fails(eng, asm, EINVAL, "last piece is N throughout", [good[0], (0, 0, 12, 0, 10, 0, 0)], [0, 2], gap=0)
        for asm in (t, pk, mz):
            fails(eng, asm, EINVAL, "holds no text", good, [0, 2])
        fails(eng, 9, EINVAL, "no assembly 9", good, [0, 2])
        # path_first must begin at 0: nodes in front of the first path would reach the unassigned side unchecked
        pf = np.array([1, 3], dtype=np.uint64)
        node = np.zeros(3, dtype=MxEngine.SCAFFOLD_NODE)
        node["start"], node["end"] = [500, 0, 0], [900, 12, 10]
        node["record"] = [0, 0, 1]
        rc = eng._lib.mxg_write_scaffolds(eng._h, a, node.ctypes.data, pf.ctypes.data, 1, -1, 0, names[0].encode(), names[1].encode(), names[2].encode(),
                                          None, None, None)
        assert rc == EINVAL and not any(os.path.exists(f) for f in names)
        with pytest.raises(ValueError, match="first one 0"):
            eng.write_scaffolds(a, node, [1, 3], assigned=names[0])
        # 2^31 nodes: refused from path_first alone, before a node is read
        pf = np.array([0, 1 << 31], dtype=np.uint64)
        node = np.zeros(2, dtype=MxEngine.SCAFFOLD_NODE)
        rc = eng._lib.mxg_write_scaffolds(eng._h, a, node.ctypes.data, pf.ctypes.data, 1, -1, 0, names[0].encode(), None, None, None, None, None)
        assert rc == ELIMIT and not os.path.exists(names[0])
        # ... and the handle still answers
        got = check_against_restatement(eng, a, records, [[("a", "+", 0, 12, 5, 0, 0), ("b", "-", 0, 10, 0, 0, 0)]], tmp_path / "ok")
        assert got[0] == b">ntJoin0\nACGTACGTNNNNNNNGTACGTACGT\n" and got[3]["lead_strip"].tolist() == [2]
    with MxEngine(k=4, w=2, drop_seq=True) as eng:
        for asm in (eng.add_fasta("t", 1.0, fasta), eng.add_records("h", 1.0, records)):
            fails(eng, asm, EINVAL, "holds no text", good, [0, 2])
    with MxEngine(k=4, w=2) as eng:  # a side-car holds a sketch, no text
        a = eng.add_fasta("t", 1.0, fasta)
        eng.sketch()
        eng.write_sketch_bin(a, str(tmp_path / "t.bin"))
        fails(eng, eng.add_bin("bin", 1.0, str(tmp_path / "t.bin")), EINVAL, "holds no text", good, [0, 2])
    # a one-shot handle gives its text back with mxg_write_outputs: both layouts work before (the host parser's text is uploaded
    # by that first call) and are refused after
    with MxEngine(k=4, w=2, one_shot=True) as eng:
        a = eng.add_fasta("t", 1.0, fasta)
        h = eng.add_records("h", 1.0, records)
        eng.sketch()
        eng.build_graph()
        for asm in (a, h):
            got = check_against_restatement(eng, asm, records, [[("a", "+", 0, 12, 5, 0, 0), ("b", "-", 0, 10, 0, 0, 0)]], tmp_path / f"y{asm}")
            assert got[0] == b">ntJoin0\nACGTACGTNNNNNNNGTACGTACGT\n"
        eng.write_outputs(str(tmp_path / "o.mx.dot"), [str(tmp_path / "a.tsv"), str(tmp_path / "h.tsv")])
        for asm in (a, h):
            fails(eng, asm, EINVAL, "holds no text", good, [0, 2])
    two = str(tmp_path / "two.fa")
    cases.write_fasta(two, [(f"r{r}", synth.to_ascii(synth.make_reference(r, 5000)[0]).decode("ascii")) for r in range(2)], 60)
    with MxEngine(k=15, w=10) as eng:
        fails(eng, eng.add_fasta_split("t", 1.0, two, 0, 2), EINVAL, "shard or pieces", good, [0, 2])


def test_state_untouched_and_repeatable(tmp_path):
    "sketches, graph and paths of the handle are what they were; a second call writes the same bytes"
    doc, fasta = cases.load_golden(os.path.join(cases.GOLDEN, "scaffolds", "f-f.overlapping.json"))
    records = _oracle.read_fasta(fasta)
    paths = cases.golden_nodes(doc)
    with MxEngine(k=32, w=100) as eng:
        a = eng.add_fasta("t", 1.0, fasta)
        b = eng.add_fasta("r", 2.0, os.path.join(cases.GOLDEN, "fasta", "ref.fa"))
        eng.sketch()
        eng.build_graph()
        found = eng.find_paths(1)
        before = (eng.get_sketch(a)["out_hash"].copy(), eng.get_sketch(b)["pos"].copy(), eng.get_graph()["vertex_hash"].copy(),
                  eng.get_graph()["edge_u"].copy())
        one = check_against_restatement(eng, a, records, paths, tmp_path / "a", 20)
        two = check_against_restatement(eng, a, records, paths, tmp_path / "b", 20)
        assert one[:3] == two[:3] and one[0] == doc["assigned"].encode("ascii")
        after = (eng.get_sketch(a)["out_hash"], eng.get_sketch(b)["pos"], eng.get_graph()["vertex_hash"], eng.get_graph()["edge_u"])
        for x, y in zip(before, after):
            assert np.array_equal(x, y)
        assert [v for _, v in eng.find_paths(1)] == [v for _, v in found]
        eng.write_tsv(a, str(tmp_path / "t.tsv"), with_pos=True, with_strand=False, with_seq=True)  # the TSV writer shares the windows


def test_one_large_call(tmp_path):
    """10^5 paths of two or three nodes over a target of 4 x 64 Mbp (256 Mbp: the restatement takes well under two minutes for it),
    lines of 80, runs of N and lower case sprinkled in, a tenth of the nodes reversed, overlap stage on; the three files by SHA-256"""
    n_rec, rec_len, n_paths, step, length = 4, 64_000_000, 104_000, 1000, 930
    rng = np.random.default_rng(5)
    seqs = []
    fasta = str(tmp_path / "big.fa")
    with open(fasta, "wb") as fh:
        for r in range(n_rec):
            text = np.frombuffer(synth.to_ascii(synth.make_reference(20 + r, rec_len)[0]), dtype=np.uint8).copy()
            for at in rng.integers(0, rec_len - 20_000, size=300).tolist():
                text[at:at + int(rng.choice([1, 7, 64, 500, 9000]))] = ord("N")
            low = rng.integers(0, rec_len - 100, size=2000)
            for at in low.tolist():
                text[at:at + 50] |= 0x20
            seqs.append((f"chr{r}", text.tobytes().decode("ascii")))
            fh.write(f">chr{r} synthetic\n".encode("ascii"))
            body = np.full((rec_len // 80, 81), ord("\n"), dtype=np.uint8)
            body[:, :80] = text.reshape(-1, 80)
            fh.write(body.tobytes())
    py = np.random.default_rng(6)
    paths, per_rec = [], rec_len // step - 4
    ori = py.random(3 * n_paths) < 0.1
    cuts = py.integers(0, 200, size=(3 * n_paths, 2))
    at, i = [0] * n_rec, 0
    for p in range(n_paths):
        r = p % n_rec
        n = 2 + (p % 3 == 0)
        if at[r] + n > per_rec:
            continue
        path = []
        for j in range(n):
            start = (at[r] + j) * step
            sa, ea = (int(cuts[i][0]) if cuts[i][0] < 100 else 0), (length - int(cuts[i][1]) if cuts[i][1] < 100 else 0)
            path.append((f"chr{r}", "-" if ori[i] else "+", start, start + length, 0 if j == n - 1 else 20 + (i % 5), sa, ea))
            i += 1
        at[r] += n
        paths.append(path)
    # a path whose first or last piece is N throughout is one the contract refuses: left out, and few
    seq_of = dict(seqs)
    generated = len(paths)
    paths = [path for path in paths if all(rs.piece(seq_of[nd[0]], nd, 20)[0].strip("Nn") for nd in (path[0], path[-1]))]
    assert generated - len(paths) <= cases.MAX_LEFT_OUT * generated and len(paths) >= 100_000, (generated, len(paths))
    t0 = time.perf_counter()
    text, leads, tails = rs.scaffolds(paths, seq_of, 20)
    bed, un_fa, n_un = rs.unassigned(seqs, paths)
    t_cpu = time.perf_counter() - t0
    with MxEngine(k=32, w=1000) as eng:
        a = eng.add_fasta("t", 1.0, fasta)
        index = {rid: r for r, (rid, _) in enumerate(seqs)}
        rows, first = cases.rows_of(paths, index)
        names = [str(tmp_path / f) for f in ("big.assigned.fa", "big.unassigned.fa", "big.bed")]
        t0 = time.perf_counter()
        res = eng.write_scaffolds(a, rows, first, overlap_gap=20, assigned=names[0], unassigned=names[1], bed=names[2])
        t_gpu = time.perf_counter() - t0
    print(f"large call: {len(paths)} paths, {len(text) / 1e6:.0f} MB assigned + {len(un_fa) / 1e6:.0f} MB unassigned: library {t_gpu:.2f} s, restatement {t_cpu:.2f} s")
    for name, want in zip(names, (text, un_fa, bed)):
        sha = hashlib.sha256()
        with open(name, "rb") as fh:
            for block in iter(lambda: fh.read(1 << 24), b""):
                sha.update(block)
        assert sha.hexdigest() == hashlib.sha256(want.encode("ascii")).hexdigest(), name
    assert res["lead_strip"].tolist() == leads and res["tail_strip"].tolist() == tails and res["n_unassigned"] == n_un
    assert sum(1 for x in leads + tails if x) > 10


# ---- the families of tests/golden/scaffolds/families: generated inputs, the reference's own print_scaffolds ------------------------

def check_pinned_to_reference(family, name, tmp_path):
    """write_scaffolds over the paths the reference answered, the last gap zeroed, on both ingest routes: the assigned FASTA record by
    record against the recorded name, length and sha256, and the strips against those the reference's .path coordinates show"""
    entry = pin.load_family(family)[name]
    case, paths = entry["case"], entry["paths"]
    fasta = str(tmp_path / "t.fa")
    cases.write_fasta(fasta, case["records"], case["width"], case["final_newline"])
    rows, first = cases.rows_of(paths, {rid: r for r, (rid, _) in enumerate(case["records"])})
    strips = [pin.reference_strips(path, line) for path, line in zip(paths, entry["path_lines"])]
    with MxEngine(k=15, w=10) as eng:
        for route, a in (("fasta", eng.add_fasta("t", 1.0, fasta)), ("records", eng.add_records("h", 1.0, case["records"]))):
            names = [str(tmp_path / (route + s)) for s in (".assigned.fa", ".unassigned.fa", ".bed")]
            res = eng.write_scaffolds(a, rows, first, overlap_gap=case["overlap_gap"], assigned=names[0], unassigned=names[1], bed=names[2])
            assert pin.scaffold_digests(read(names[0]).decode("ascii")) == entry["scaffolds"], route
            assert list(zip(res["lead_strip"].tolist(), res["tail_strip"].tolist())) == strips, route


@pytest.mark.parametrize("seed", cases.FUZZ_SEEDS)
def test_fuzz_pinned_to_reference(seed, tmp_path):
    check_pinned_to_reference("fuzz", f"seed{seed:02d}", tmp_path)


@pytest.mark.parametrize("name", [name for name, _g, _a in pin.family_specs()["strip_beside_cuts"]])
def test_strip_beside_cuts_pinned_to_reference(name, tmp_path):
    "a strip that moves a coordinate in a path whose other nodes carry cuts and replaced gaps: the only such answers ntJoin gives"
    check_pinned_to_reference("strip_beside_cuts", name, tmp_path)


@pytest.mark.parametrize("name", [name for name, _g, _a in pin.family_specs()["agp_names"]])
def test_agp_names_pinned_to_reference(name, tmp_path):
    check_pinned_to_reference("agp_names", name, tmp_path)


PIN_CASES = pin.all_cases()


@pytest.mark.parametrize("family,name", PIN_CASES, ids=[f"{family}-{name}" for family, name in PIN_CASES])
def test_families_end_to_end_through_print_scaffolds(family, name, tmp_path, monkeypatch):
    """Ntjoin.print_scaffolds over a target loaded from the case's FASTA: the assigned FASTA, the .path and the AGP (assigned and
    unassigned lines) are the reference's bytes for all pinned paths, also where the writer refuses an inverted interval and
    _write_path_host writes both files.  The nodes go in as format_paths() gives them: print_scaffolds zeroes the last gap itself."""
    entry = pin.load_family(family)[name]
    case = entry["case"]
    monkeypatch.chdir(tmp_path)
    cases.write_fasta("t.fa", case["records"], case["width"], case["final_newline"])
    on = case["overlap_gap"] is not None
    paths9 = [pin.rows9(case["paths"][p]) for p in entry["pinned"]]
    adjust = [[(nd[5], nd[6]) for nd in path] for path in entry["paths"]] if on else None
    with MxEngine(k=15, w=10) as eng:
        eng.add_fasta(pin.TARGET, 1.0, "t.fa")
        nj = Ntjoin.__new__(Ntjoin)
        nj._engine, nj._order, nj._fasta, nj.args = eng, [pin.TARGET], {pin.TARGET: "t.fa"}, argparse.Namespace(p="out")
        host = []
        monkeypatch.setattr(nj, "_write_path_host", lambda *a, _host=nj._write_path_host: (host.append(1), _host(*a))[1])
        files = nj.print_scaffolds(paths9, adjust, n=1, agp=True, overlap_gap=case["overlap_gap"] if on else 20)
    assert files["assigned"] == "t.fa.k15.w10.n1.assigned.scaffolds.fa" and files["path"] == "out.path" and files["agp"] == "out.agp"
    assert pin.scaffold_digests(read(files["assigned"]).decode("ascii")) == entry["scaffolds"]
    assert read(files["path"]) == entry["path"].encode("ascii")
    assert read(files["agp"]) == (entry["agp"] + entry["agp_unassigned"]).encode("ascii")
    assert bool(host) == bool(pin.refused_nodes(entry))   # the host loop wrote the files exactly where an interval is inverted
