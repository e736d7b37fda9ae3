"""GPU tests of the overlap stage's cut points (mxg_overlap_cuts, csrc/overlap.hip; reference adjust_for_trimming,
bin/ntjoin_assemble.py:468-516, and merge_overlapping, bin/ntjoin_overlap.py:20-88): the goldens (the reference's own output) through
the C-ABI and through Ntjoin.trim_overlaps, seeded fuzz and a call with 10^5 junctions against the restatement
(tests/_overlap_restatement.py), small scratch batches = one batch, the argument errors, and the handle's state untouched.
Integers only: every comparison is exact."""
import argparse
import glob
import os
import random

import numpy as np
import pytest

from ntjoin_amd import synth
from ntjoin_amd.engine import MxEngine, MxError
from ntjoin_amd.ntjoin import Ntjoin
from tests import _oracle, _overlap_restatement as rs
from tests._overlap_cases import load_case

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
CASES = sorted(glob.glob(os.path.join(GOLDEN, "overlap", "*.json")))
IDS = [os.path.basename(c)[:-5] for c in CASES]
EINVAL, ELIMIT = -1, -5


def flat(paths, index):
    "paths of (contig, ori, start, end, raw_gap) -> rows for MxEngine.overlap_cuts, path_first"
    rows, first = [], [0]
    for path in paths:
        rows.extend((index[c], s, e, g, o == "-") for c, o, s, e, g in path)
        first.append(len(rows))
    return rows, first


def unflat(arr, first):
    return [arr[a:b].tolist() for a, b in zip(first[:-1], first[1:])]


def oracle_sketch(variant=_oracle.V2_SUM):
    orc = _oracle.load()
    return lambda text, k, w: [(h, p) for h, p, _f, _m in orc.sketch(text, k, w, variant)]


def check_against_restatement(eng, a, records, paths, k, w, variant=_oracle.V2_SUM):
    index = {rid: r for r, (rid, _) in enumerate(records)}
    rows, first = flat(paths, index)
    got = eng.overlap_cuts(a, rows, first, k=k, w=w)
    sa, ea, cf, _ = rs.cuts(paths, dict(records), k, w, oracle_sketch(variant))
    assert unflat(got["start_adjust"], first) == sa
    assert unflat(got["end_adjust"], first) == ea
    assert unflat(got["cut_found"], first) == cf
    return got


@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("route", ["fasta", "buffers"])
def test_goldens_through_the_c_abi(case, route):
    doc, fasta = load_case(case)
    records = _oracle.read_fasta(fasta)
    with MxEngine(k=32, w=1000) as eng:  # (the handle's k and w are not the call's)
        a = eng.add_fasta("t", 1.0, fasta) if route == "fasta" else eng.add_records("t", 1.0, records)
        index = {rid: r for r, (rid, _) in enumerate(records)}
        rows, first = flat([[(nd[0], nd[1], nd[2], nd[3], nd[8]) for nd in p] for p in doc["paths"]], index)
        got = eng.overlap_cuts(a, rows, first, k=doc["meta"]["k"], w=doc["meta"]["w"])
    assert unflat(got["start_adjust"], first) == doc["start_adjust"]
    assert unflat(got["end_adjust"], first) == doc["end_adjust"]
    assert unflat(got["cut_found"], first) == doc["cut_found"]
    if "reference_path" in doc["meta"]:
        line = rs.path_string(doc["paths"][0], got["start_adjust"].tolist(), got["end_adjust"].tolist())
        assert line == doc["meta"]["reference_path"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_goldens_through_trim_overlaps(case, tmp_path):
    doc, fasta = load_case(case)
    tgt = str(tmp_path / "tgt.fa.k32.w100.tsv")
    args = argparse.Namespace(k=32, FILES=[], s=tgt, l=1.0, p=str(tmp_path / "out"), n=1, overlap_k=doc["meta"]["k"],
                              overlap_w=doc["meta"]["w"])
    nj = Ntjoin(args, fasta={tgt: fasta}, w=100)
    try:
        nj.load_minimizers_scaffold()
        # '?' nodes and paths left with one node are dropped, as print_scaffolds drops them
        first = doc["paths"][0]
        extra = [first[0][:1] + ["?"] + first[0][2:]]
        paths = [p[:1] + extra + p[1:] for p in doc["paths"]] + [[first[0]], [first[0], extra[0]]]
        got = nj.trim_overlaps(paths)
        assert got[len(doc["paths"]):] == [[], []]
        for res, sa, ea in zip(got, doc["start_adjust"], doc["end_adjust"]):
            assert res == list(zip(sa, ea))
        if doc["meta"]["k"] == 15:
            args.overlap_k = args.overlap_w = None  # the reference's defaults: 15, 10
            assert nj.trim_overlaps(doc["paths"]) == got[:len(doc["paths"])]
    finally:
        nj.close()


def test_trim_overlaps_needs_bases(tmp_path):
    _, fasta = load_case(CASES[0])
    orc = _oracle.load()
    tsv = str(tmp_path / "t.fa.k32.w100.tsv")
    orc.fasta_to_tsv(fasta, tsv, 32, 100)
    nj = Ntjoin(argparse.Namespace(k=32, FILES=[], s=tsv, l=1.0, p=str(tmp_path / "o"), n=1))
    try:
        nj.load_minimizers_scaffold()
        with pytest.raises(ValueError, match="TSV"):
            nj.trim_overlaps([])
    finally:
        nj.close()


def fuzz_input(seed, n_paths, alphabet="ACGT"):
    "paths over overlapping windows of random contigs: true overlaps, wrong estimates, N islands, all orientations"
    rng = random.Random(seed)
    records, paths = [], []
    comp = str.maketrans("ACGT", "TGCA")
    for p in range(n_paths):
        genome = "".join(rng.choice(alphabet) for _ in range(rng.randint(400, 6000)))
        if rng.random() < 0.3:
            unit = genome[50:50 + rng.randint(12, 40)]
            at = rng.randint(100, len(genome) - 100)
            genome = genome[:at] + unit * 3 + genome[at:]
        if rng.random() < 0.4:
            g = list(genome)
            for _ in range(rng.randint(1, 4)):
                at = rng.randint(0, len(g) - 1)
                for q in range(at, min(len(g), at + rng.choice([1, 2, 9, 30]))):
                    g[q] = "N"
            genome = "".join(g)
        n_nodes = rng.randint(2, 9)
        step = max(30, len(genome) // (n_nodes + 1))
        nodes, lo = [], 0
        for i in range(n_nodes):
            hi = min(len(genome), lo + step + rng.randint(5, step))
            while lo < hi and genome[lo] == "N":
                lo += 1
            while hi > lo and genome[hi - 1] == "N":
                hi -= 1
            if hi - lo < 2:
                break
            nxt = max(lo + 1, hi - rng.randint(1, min(step, hi - lo)))
            true_ov = hi - nxt
            gap = rng.choice([-true_ov, -true_ov, -true_ov - 7, -max(1, true_ov - 5), -(hi - lo) - 40, 25, -1])
            ori = rng.choice("+-")
            piece = genome[lo:hi]
            if rng.random() < 0.3:  # a diverged copy
                piece = "".join(rng.choice("ACGT") if c != "N" and rng.random() < 0.03 else c for c in piece)
            pad = "".join(rng.choice("ACGT") for _ in range(rng.choice([0, 3, 21])))
            cid = f"f{p}_{i}"
            records.append((cid, pad + (piece if ori == "+" else piece.translate(comp)[::-1]) + pad))
            nodes.append((cid, ori, len(pad), len(pad) + len(piece), gap))
            lo = nxt
        if len(nodes) >= 2:
            paths.append(nodes)
    return records, paths


@pytest.mark.parametrize("k,w,variant,seed,n_paths", [(15, 10, "v2", 1, 400), (15, 10, "v1", 2, 120), (32, 64, "v2", 3, 150), (11, 1, "v2", 4, 80),
                                                    (21, 300, "v2", 5, 80), (4, 5, "v2", 6, 80)])
def test_fuzz_against_restatement(k, w, variant, seed, n_paths):
    records, paths = fuzz_input(seed, n_paths)
    with MxEngine(k=32, w=50, variant=variant) as eng:
        a = eng.add_records("t", 1.0, records)
        got = check_against_restatement(eng, a, records, paths, k, w, _oracle.V1_MIN if variant == "v1" else _oracle.V2_SUM)
    if (k, w) == (15, 10):
        assert got["cut_found"].sum() > 50


def test_small_batches_equal_one_batch(monkeypatch):
    "MXG_OVL_BATCH: the scratch budget in list entries; tiny budgets work through the paths a few at a time"
    doc, fasta = load_case(os.path.join(GOLDEN, "overlap", "synth_k15_w10.json"))
    records = _oracle.read_fasta(fasta)
    index = {rid: r for r, (rid, _) in enumerate(records)}
    rows, first = flat([[(nd[0], nd[1], nd[2], nd[3], nd[8]) for nd in p] for p in doc["paths"]], index)
    res = []
    for budget in (None, "1", "5000"):
        if budget is None:
            monkeypatch.delenv("MXG_OVL_BATCH", raising=False)
        else:
            monkeypatch.setenv("MXG_OVL_BATCH", budget)
        with MxEngine(k=32, w=100) as eng:
            a = eng.add_records("t", 1.0, records)
            res.append(eng.overlap_cuts(a, rows, first))
            if budget:
                assert f"MXG_OVL_BATCH={budget}" in eng.knobs()
    for r in res[1:]:
        for key in ("start_adjust", "end_adjust", "cut_found"):
            assert np.array_equal(r[key], res[0][key])
    assert unflat(res[0]["end_adjust"], first) == doc["end_adjust"]


@pytest.mark.parametrize("case", [c for c in CASES if "synth" in c], ids=[i for i in IDS if "synth" in i])
def test_forced_routes_equal_default(case, monkeypatch):
    "MXG_OVL_PAIRWISE: 0 = every list through the hash table (the general route), a huge value = every list pairwise"
    doc, fasta = load_case(case)
    records = _oracle.read_fasta(fasta)
    index = {rid: r for r, (rid, _) in enumerate(records)}
    rows, first = flat([[(nd[0], nd[1], nd[2], nd[3], nd[8]) for nd in p] for p in doc["paths"]], index)
    for knob in ("0", "1000000000", None):
        if knob is None:
            monkeypatch.delenv("MXG_OVL_PAIRWISE", raising=False)
        else:
            monkeypatch.setenv("MXG_OVL_PAIRWISE", knob)
        with MxEngine(k=32, w=100) as eng:
            a = eng.add_records("t", 1.0, records)
            got = eng.overlap_cuts(a, rows, first, k=doc["meta"]["k"], w=doc["meta"]["w"])
            assert (knob is None) or f"MXG_OVL_PAIRWISE={knob}" in eng.knobs()
        assert unflat(got["start_adjust"], first) == doc["start_adjust"]
        assert unflat(got["end_adjust"], first) == doc["end_adjust"]
        assert [[int(c) for c in v] for v in unflat(got["cut_found"], first)] == [[int(c) for c in v] for v in doc["cut_found"]]


def test_long_overlaps():
    """overlaps of 120 000 bases (about 2 * 10^4 minimizers per list: the table route), one estimated beyond the segments so
    that whole contigs are kept ends, a repeat inside, a diverged copy; against the restatement"""
    rng = random.Random(77)
    comp = str.maketrans("ACGT", "TGCA")
    g = "".join(rng.choice("ACGT") for _ in range(330_000))
    g = g[:100_000] + g[60_000:60_300] + g[100_000:]  # a repeated unit inside the first overlap
    b = "".join(rng.choice("ACGT") if rng.random() < 0.002 else c for c in g[30_000:180_000])
    records = [("a", g[:150_000]), ("b", b.translate(comp)[::-1]), ("c", g[60_000:210_000]), ("d", g[180_000:330_000])]
    paths = [[("a", "+", 0, 150_000, -120_000), ("b", "-", 0, 150_000, -120_000), ("c", "+", 0, 150_000, 0)],
             [("c", "+", 0, 150_000, -400_000), ("d", "+", 0, 150_000, -7)]]
    with MxEngine(k=32, w=100) as eng:
        a = eng.add_records("t", 1.0, records)
        got = check_against_restatement(eng, a, records, paths, 15, 10)
    assert got["cut_found"].tolist() == [True, True, False, True, False]


def test_accepted_maxima_of_k_and_w():
    """k = 256 and w = 4096, the largest the call takes (257 and 4097 are refused: test_errors_and_state_untouched): one junction
    of two contigs that overlap by 30 000 bases, against the restatement"""
    rng = random.Random(256)
    g = "".join(rng.choice("ACGT") for _ in range(90_000))
    records = [("a", g[:60_000]), ("b", g[30_000:])]
    paths = [[("a", "+", 0, 60_000, -30_000), ("b", "+", 0, 60_000, 0)]]
    with MxEngine(k=32, w=100) as eng:
        a = eng.add_records("t", 1.0, records)
        got = check_against_restatement(eng, a, records, paths, 256, 4096)
    assert got["cut_found"].tolist() == [True, False]


def test_pieces_are_refused(tmp_path):
    fasta = str(tmp_path / "two.fa")
    rng = random.Random(5)
    with open(fasta, "w", encoding="ascii") as fh:
        for r in range(2):
            fh.write(f">r{r}\n" + "".join(rng.choice("ACGT") for _ in range(5000)) + "\n")
    with MxEngine(k=15, w=10) as eng:
        a = eng.add_fasta_split("t", 1.0, fasta, 0, 2)
        with pytest.raises(MxError, match="pieces") as ei:
            eng.overlap_cuts(a, [(0, 0, 2000, -100, 0), (0, 1900, 4000, 0, 0)], [0, 2])
        assert ei.value.code == EINVAL


def test_many_junctions():
    "one call with more than 10^5 junctions on bases handed over packed in HBM; a seeded sample of 500 against the restatement; a second call gives the same arrays"
    n_nodes, step, length = 110_000, 500, 1000
    codes = synth.make_reference(11, step * n_nodes + length)[0]
    text = synth.to_ascii(codes).decode("ascii")
    rng = random.Random(12)
    rows, first, paths = [], [0], []
    i = 0
    while i + 2 <= n_nodes:
        n = min(rng.randint(2, 20), n_nodes - i)
        path = []
        for j in range(i, i + n):
            path.append(("g", "-" if rng.random() < 0.1 else "+", j * step, j * step + length, -(length - step) - rng.choice([0, 0, 3])))
        paths.append(path)
        rows.extend((0, s, e, g, o == "-") for _, o, s, e, g in path)
        first.append(len(rows))
        i += n
    junctions = len(rows) - len(paths)
    assert junctions >= 100_000
    import torch
    words, rec_start, rec_len = synth.pack_records([codes])
    d_words = torch.from_numpy(words.view(np.int32)).cuda()
    with MxEngine(k=32, w=1000) as eng:  # bases handed over in HBM: no invalid bases, no text
        a = eng.add_packed_device("t", 1.0, d_words.data_ptr(), rec_start, rec_len, ids=["g"], keepalive=d_words)
        got = eng.overlap_cuts(a, rows, first)
        again = eng.overlap_cuts(a, rows, first)
    for key in got:
        assert np.array_equal(got[key], again[key])
    assert got["cut_found"].sum() > junctions // 2
    sample = rng.sample(range(len(paths)), 60)
    sub = [paths[p] for p in sample]
    assert sum(len(p) - 1 for p in sub) >= 500
    sa, ea, cf, _ = rs.cuts(sub, {"g": text}, 15, 10, oracle_sketch())
    for p, s, e, c in zip(sample, sa, ea, cf):
        lo, hi = first[p], first[p + 1]
        assert got["start_adjust"][lo:hi].tolist() == s and got["end_adjust"][lo:hi].tolist() == e
        assert got["cut_found"][lo:hi].tolist() == c


def test_errors_and_state_untouched(tmp_path):
    doc, fasta = load_case(os.path.join(GOLDEN, "overlap", "f-f.overlapping.json"))
    records = _oracle.read_fasta(fasta) + [("withN", "ACGTNACGTACGTACGTACGTNNACGT")]
    orc = _oracle.load()
    tsv = str(tmp_path / "x.fa.k32.w100.tsv")
    orc.fasta_to_tsv(fasta, tsv, 32, 100)
    good = [(0, 0, 2099, -100, 0), (1, 0, 2331, 0, 0)]
    with MxEngine(k=32, w=100) as eng:
        a = eng.add_records("t", 1.0, records)
        b = eng.add_tsv("tsv", 1.0, tsv)
        eng.sketch()
        eng.build_graph()
        found = eng.find_paths(1)
        before = (eng.get_sketch(a)["out_hash"].copy(), eng.get_sketch(a)["pos"].copy(), eng.get_graph()["vertex_hash"].copy(),
                  eng.get_graph()["edge_u"].copy())
        res = eng.overlap_cuts(a, good, [0, 2])
        assert res["end_adjust"].tolist() == [2033, 0] and res["start_adjust"].tolist() == [0, 34]

        def fails(code, match, nodes, pf, asm=a, k=15, w=10):
            with pytest.raises(MxError, match=match) as ei:
                eng.overlap_cuts(asm, nodes, pf, k=k, w=w)
            assert ei.value.code == code

        fails(EINVAL, "minimizer table", good, [0, 2], asm=b)
        fails(EINVAL, "path 0 node 1", [good[0], (1, 50, 50, 0, 0)], [0, 2])
        fails(EINVAL, "path 0 node 1", [good[0], (1, 0, 2332, 0, 0)], [0, 2])
        fails(EINVAL, "path 1 has 1 node", good + [good[0]], [0, 2, 3])
        fails(EINVAL, "path 0 node 1.*invalid base", [good[0], (2, 0, 5, 0, 0)], [0, 2])
        fails(EINVAL, "path 0 node 1.*invalid base", [good[0], (2, 5, 22, 0, 0)], [0, 2])
        fails(EINVAL, "record 9", [good[0], (9, 0, 5, 0, 0)], [0, 2])
        fails(ELIMIT, "256", good, [0, 2], k=257)
        fails(ELIMIT, "4096", good, [0, 2], w=4097)
        assert eng.overlap_cuts(a, good, [0, 2], k=32, w=64)["cut_found"].tolist() == [True, False]
        empty = eng.overlap_cuts(a, np.zeros(0, dtype=MxEngine.OVERLAP_NODE), [0])
        assert len(empty["cut_found"]) == 0
        after = (eng.get_sketch(a)["out_hash"], eng.get_sketch(a)["pos"], eng.get_graph()["vertex_hash"], eng.get_graph()["edge_u"])
        for x, y in zip(before, after):
            assert np.array_equal(x, y)
        assert [v for _, v in eng.find_paths(1)] == [v for _, v in found]
