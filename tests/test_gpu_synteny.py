"""GPU tests of mxg_synteny_blocks and mxg_write_synteny_paf (include/ntjoin_mx.h, row f12) against the sequential restatement of
the contract (tests/_synteny_restatement.py) applied to the arrays of mxg_get_graph: the hand-made cases and the seeded fuzz of
tests/_synteny_cases.py, anchor counts around the wave, the 256-thread block, the 1024-element tile of the scans and past 2^16,
single blocks, a zigzag of turning points, a list without links, the filters, piece tables of every shape, three assemblies, every
refusal with the handle usable afterwards, and the PAF text byte for byte at several window sizes."""
import random

import numpy as np
import pytest

from tests import _synteny_cases as cases, _synteny_restatement as R

pytestmark = pytest.mark.gpu

HAND = cases.hand_cases()


def load(case, **engine_kw):
    from ntjoin_amd.engine import MxEngine
    eng = MxEngine(k=case["k"], w=10, **engine_kw)
    for a, asm in enumerate(case["asms"]):
        hs = [h for _rid, mxs in asm for h, _p in mxs]
        ps = [p for _rid, mxs in asm for _h, p in mxs]
        rs = [r for r, (_rid, mxs) in enumerate(asm) for _ in mxs]
        eng.add_minimizers(f"asm{a}", 1.0, np.array(hs, dtype=np.uint64), np.array(ps, dtype=np.uint32), np.array(rs, dtype=np.uint32),
                           [rid for rid, _mxs in asm])
    eng.build_graph()
    return eng


def device(eng, case, **over):
    c = dict(case, **over)
    return eng.synteny_blocks(c["q"], c["s"], max_gap=c["max_gap"], min_anchors=c["min_anchors"], min_span=c["min_span"], pieces=c["pieces"],
                              first=c["first"], query_length=c["lengths"][c["q"]], subject_length=c["lengths"][c["s"]])


def restated(eng, case, **over):
    "the restatement over the graph arrays the handle itself reports"
    c = dict(case, **over)
    g = eng.get_graph()
    return R.synteny(g["vertex_pos"], g["vertex_record"], c["q"], c["s"], c["k"], c["max_gap"], c["min_anchors"], c["min_span"], c["pieces"],
                     c["first"])


def as_tuples(got):
    return list(zip(*[got[name].tolist() for name in R.FIELDS]))


def check(eng, case, **over):
    got, want = device(eng, case, **over), restated(eng, case, **over)
    assert (got["n_anchors_total"], got["n_links"], got["n_blocks"]) == (want["n_anchors_total"], want["n_links"], len(want["blocks"]))
    assert as_tuples(got) == want["blocks"]
    return want


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases(name):
    case = HAND[name]
    with load(case) as eng:
        want = check(eng, case)
    assert want["blocks"] == case["expect"]


def test_fuzz():
    "100 seeded cases: three assemblies, drop-outs, strays, every other one through a random piece table"
    blocks = 0
    for i in range(cases.FUZZ_CASES):
        case = cases.fuzz_case(i)
        with load(case) as eng:
            blocks += len(check(eng, case)["blocks"])
    assert blocks > 200


@pytest.mark.parametrize("n", [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 65537])
def test_anchor_counts(n):
    "the wave, the 256-thread block, the 1024-element tile, one past 2^16; with and without the filters and a table of one piece per record"
    case = cases.mixed_case(n, seed=n + 1)
    with load(case) as eng:
        want = check(eng, case)
        assert want["n_anchors_total"] == n
        check(eng, case, max_gap=900, min_anchors=3)
        lengths = case["lengths"][1]
        check(eng, case, pieces=[(r, 0, ln, r % 2) for r, ln in enumerate(lengths)], first=list(range(len(lengths) + 1)))


@pytest.mark.parametrize("reverse", [False, True])
def test_one_block_over_all_anchors(reverse):
    case = cases.line_case(4097, reverse=reverse)
    with load(case) as eng:
        want = check(eng, case)
    assert want["blocks"] == [(4097, 0, 0, 50 * 4096 + 32, 0, 0, 70 * 4096 + 32, int(reverse))]


def test_zigzag_every_anchor_a_turning_point():
    case = cases.zigzag_case(1025)
    with load(case) as eng:
        want = check(eng, case)
        assert len(want["blocks"]) == 1024 and all(b[0] == 2 for b in want["blocks"])
        assert device(eng, case, min_anchors=3)["n_blocks"] == 0


def test_no_link_at_all():
    case = cases.nolink_case(1025)
    with load(case) as eng:
        want = check(eng, case)
    assert want == {"n_anchors_total": 1025, "n_links": 0, "blocks": []}


def test_filters():
    case = cases.mixed_case(3000, seed=8)
    with load(case) as eng:
        kept = [len(check(eng, case, min_anchors=m)["blocks"]) for m in (2, 3, 5)]
        assert kept[0] > kept[1] > kept[2] > 0
        spans = [len(check(eng, case, min_span=sp)["blocks"]) for sp in (0, 500, 20000)]
        assert spans[0] > spans[1] > spans[2]
        check(eng, case, max_gap=100)
        check(eng, case, max_gap=899)
        check(eng, case, max_gap=900)


def test_piece_tables():
    "a record of 1000 pieces, records of one piece, pieces without anchors, GAP pieces, piece counts at the block and tile borders"
    case = cases.mixed_case(3000, seed=4)
    rng = random.Random(11)
    with load(case) as eng:
        pieces, first = cases.pieces_of(case, rng, many=1000)
        assert first[1] - first[0] >= 1000 and any(p[3] == R.GAP for p in pieces)
        check(eng, case, pieces=pieces, first=first)
        for trial in range(6):
            pieces, first = cases.pieces_of(case, rng)
            check(eng, case, pieces=pieces, first=first)
        ln = case["lengths"][1][0]
        for n in (1, 255, 256, 257, 1023, 1024, 1025):   # n pieces over record 0, each its own table record; every other one reversed
            at = [ln * i // n for i in range(n + 1)]
            check(eng, case, pieces=[(0, lo, hi, i % 2) for i, (lo, hi) in enumerate(zip(at, at[1:]))], first=list(range(n + 1)))
        # pieces that take nothing: shorter than k, and gaps only
        none = check(eng, case, pieces=[(0, 0, 31, R.FWD), (0, 0, 10, R.GAP), (0, 5, 20, R.REV)], first=[0, 2, 3])
        assert none == {"n_anchors_total": 0, "n_links": 0, "blocks": []}
        assert check(eng, case, pieces=[], first=[0])["n_anchors_total"] == 0


def test_three_assemblies_either_subject():
    case = cases.mixed_case(700, seed=5, extra_asm=True)
    assert len(case["asms"]) == 3
    with load(case) as eng:
        a = check(eng, case, q=1, s=0)
        b = check(eng, case, q=1, s=2)
        c = check(eng, case, q=2, s=1)
        d = check(eng, case, q=0, s=1)
    # (the third assembly holds the minimizers in the query's own order: forward blocks only, broken at the query's record borders)
    assert a["blocks"] != b["blocks"] and all(blk[7] == 0 for blk in b["blocks"]) and len(b["blocks"]) <= len(case["asms"][1])
    assert c["blocks"] and d["blocks"]


def test_handle_lengths_are_needed_where_the_handle_holds_none():
    from ntjoin_amd import capi
    from ntjoin_amd.engine import MxError
    case = HAND["turning_point"]
    with load(case) as eng:
        for kw in (dict(), dict(query_length=case["lengths"][1]), dict(subject_length=case["lengths"][0])):
            with pytest.raises(MxError) as err:
                eng.synteny_blocks(1, 0, min_anchors=2, **kw)
            assert err.value.code == capi.MXG_EINVAL and "holds no record lengths" in str(err.value)
        check(eng, case)


def test_refusals_leave_the_handle_usable():
    import ctypes as C

    from ntjoin_amd import capi
    from ntjoin_amd.engine import MxEngine, MxError
    case = HAND["rev_piece"]
    ql, sl = case["lengths"][1], case["lengths"][0]

    def refused(eng, code, word, **kw):
        args = dict(q=1, s=0, min_anchors=2, query_length=ql, subject_length=sl)
        args.update(kw)
        q, s = args.pop("q"), args.pop("s")
        with pytest.raises(MxError) as err:
            eng.synteny_blocks(q, s, **args)
        assert err.value.code == code and word in str(err.value), str(err.value)

    with MxEngine(k=32, w=10) as eng:   # no graph
        eng.add_minimizers("a", 1.0, np.array([5], dtype=np.uint64), np.array([1], dtype=np.uint32), np.array([0], dtype=np.uint32), ["r"])
        eng.add_minimizers("b", 1.0, np.array([5], dtype=np.uint64), np.array([1], dtype=np.uint32), np.array([0], dtype=np.uint32), ["r"])
        refused(eng, capi.MXG_EINVAL, "mxg_build_graph", query_length=[100], subject_length=[100])
        with pytest.raises(MxError) as err:
            eng.write_synteny_paf("/dev/null")
        assert err.value.code == capi.MXG_EINVAL
    with load(case) as eng:
        refused(eng, capi.MXG_EINVAL, "both assembly", q=1, s=1, subject_length=ql)
        refused(eng, capi.MXG_EINVAL, "out of range", q=2)
        refused(eng, capi.MXG_EINVAL, "out of range", s=-1)
        refused(eng, capi.MXG_EINVAL, "at least two", min_anchors=1)
        refused(eng, capi.MXG_EINVAL, "at least two", min_anchors=0)
        for pieces, first, code, word in (([(0, 50, 5000, R.REV)], [0, 1], capi.MXG_EINVAL, "query record 0 piece 0 {0, 50, 5000, 1} is not inside"),
                                          ([(0, 60, 60, R.FWD)], [0, 1], capi.MXG_EINVAL, "empty or inverted"),
                                          ([(7, 0, 10, R.FWD)], [0, 1], capi.MXG_EINVAL, "does not exist"),
                                          ([(0, 0, 10, 3)], [0, 1], capi.MXG_EINVAL, "unknown kind"),
                                          ([(0, 0, 10, R.FWD)], [0, 1, 1], capi.MXG_EINVAL, "has no pieces"),
                                          ([(0, 0, 10, R.FWD)], [1, 1], capi.MXG_EINVAL, "does not start at 0"),
                                          ([(0, 0, 2 ** 32 - 1, R.GAP), (0, 0, 1, R.GAP)], [0, 2], capi.MXG_ELIMIT, "longer than 2^32 - 1")):
            refused(eng, code, word, pieces=np.array(pieces, dtype=np.uint32).reshape(-1, 4), first=first)
        # struct_size too small, through the C entry itself
        p = capi.SyntenyParams(8, 0, 2, 0)
        v = capi.SyntenyView()
        lens = np.array(ql, dtype=np.uint32)
        rc = eng._lib.mxg_synteny_blocks(eng._h, 1, 0, C.byref(p), None, None, 0, lens.ctypes.data, lens.ctypes.data, C.byref(v))
        assert rc == capi.MXG_EINVAL and b"struct_size" in eng._lib.mxg_last_error(eng._h)
        # a table's records have no names in the handle
        device(eng, case)
        with pytest.raises(MxError) as err:
            eng.write_synteny_paf("/dev/null")
        assert err.value.code == capi.MXG_EINVAL and "pass their names" in str(err.value)
        assert check(eng, case)["blocks"] == case["expect"]
        g = eng.get_graph()
        assert g["vertex_pos"].shape == (2, 3) and eng.sketch_size(0) == 3   # graph and sketches as they were


def paf_case(n=3000):
    "about n lines (a zigzag) over several records with names of 1 to 40 bytes, through a table so that the names are the caller's"
    case = cases.from_anchors([(i // 600, 50 * (i % 600), i // 900, 1000 + (i % 2) * 500 + i) for i in range(n)])
    lengths = case["lengths"][1]
    case["pieces"] = [(r, 0, ln, r % 2) for r, ln in enumerate(lengths)]
    case["first"] = list(range(len(lengths) + 1))
    case["names"] = ["q" * (1 + 13 * r % 40) + str(r) for r in range(len(lengths))]
    return case


def write_paf(case, path, n_refs=1):
    with load(case) as eng:
        want = ""
        for j in range(n_refs):
            w = check(eng, case)
            eng.write_synteny_paf(path, query_names=case["names"], append=j > 0)
            want += R.paf(w["blocks"], case["names"], R.query_lengths(case["lengths"][1], case["pieces"], case["first"]),
                          [rid for rid, _ in case["asms"][0]], case["lengths"][0], case["k"])
        knobs = eng.knobs()
    with open(path, "rb") as fh:
        return fh.read(), want.encode("ascii"), knobs


def test_paf_text_and_append(tmp_path):
    case = paf_case()
    got, want, _ = write_paf(case, tmp_path / "a.paf")
    assert got == want and got.count(b"\n") > 1000
    twice, want2, _ = write_paf(case, tmp_path / "b.paf", n_refs=2)
    assert twice == want2 == want + want
    # a turning point on the handle's own names, without a table; no blocks: an empty file
    hand = HAND["turning_point"]
    with load(hand) as eng:
        device(eng, hand)
        eng.write_synteny_paf(tmp_path / "c.paf")
        device(eng, hand, min_anchors=4)
        eng.write_synteny_paf(tmp_path / "d.paf")
    assert (tmp_path / "c.paf").read_text() == "rec0\t632\t100\t332\t+\trec0\t3132\t1000\t3032\t96\t2032\t255\tcm:i:3\n" \
                                               "rec0\t632\t300\t532\t-\trec0\t3132\t2200\t3032\t96\t832\t255\tcm:i:3\n"
    assert (tmp_path / "d.paf").read_bytes() == b""


@pytest.mark.parametrize("win", ["1", "7", "4096"])
def test_small_windows_equal_the_default(win, tmp_path, monkeypatch):
    "MXG_SYN_WIN: bytes of PAF text per device window, parsed once per handle: a fresh handle each time"
    case = paf_case(300 if win == "7" else 3000)
    if win == "1":   # (one launch per byte: a shorter text)
        case = dict(HAND["record_borders"], names=None)
        case["pieces"], case["first"], case["names"] = [(0, 0, 172, 0), (1, 0, 157, 0)], [0, 1, 2], ["first", "second_record"]
    default, want, knobs = write_paf(case, tmp_path / "default.paf")
    assert default == want and "MXG_SYN_WIN" not in knobs
    monkeypatch.setenv("MXG_SYN_WIN", win)
    got, _, knobs = write_paf(case, tmp_path / "win.paf")
    assert f"MXG_SYN_WIN={win}" in knobs
    assert got == default and len(got) > 3 * int(win)
