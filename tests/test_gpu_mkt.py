"""GPU tests of the --mkt statistics (reference bin/ntjoin_assemble.py:37-40, pymannkendall.original_test on every run that is
not strictly monotone): mxg_mk_stats against independent numpy oracles and closed forms at the tile boundaries of the merge
sort (csrc/mk.hip), mxg_path_segments_mk and Ntjoin.format_paths(mkt=True) against a host restatement on synthetic
assemblies built to need the test, the goldens (all monotone) unchanged, and the errors."""
import argparse
import contextlib
import io
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN, golden_cases, load_case

pytestmark = pytest.mark.gpu

T = 2048  # csrc/mk.hip MK_TILE: values per LDS tile, the width of the first global merge level


def _sign_matrix(x):
    """s and tie term of one run from the pairwise sign matrix (chunked; meant for n <= 3e4)"""
    x = np.asarray(x, dtype=np.int64)
    n, s = len(x), 0
    for i0 in range(0, n, 512):
        blk = x[i0:i0 + 512]
        tri = np.triu(np.ones((len(blk), len(blk)), dtype=bool), 1)
        s += int(((blk[None, :] > blk[:, None]) & tri).sum()) - int(((blk[None, :] < blk[:, None]) & tri).sum())
        rest = x[i0 + len(blk):]
        if len(rest):
            s += int((rest[None, :] > blk[:, None]).sum()) - int((rest[None, :] < blk[:, None]).sum())
    return s, _tie_term(x)


def _tie_term(x):
    _, c = np.unique(np.asarray(x), return_counts=True)
    return sum(int(t) * (int(t) - 1) * (2 * int(t) + 5) for t in c.tolist())


def _merge_count(x):
    """s of one run by a vectorised bottom-up merge in numpy (any n): pad to a power of two with values above all others
    (they follow every real value, so they add n * pads concordant pairs), then per level every right block's values count
    the left block's smaller and larger values by searchsorted over row-offset keys"""
    x = np.asarray(x, dtype=np.int64)
    n = len(x)
    if n < 2:
        return 0
    size = 1 << (n - 1).bit_length()
    big = int(x.max()) + 1
    a = np.concatenate([x, np.full(size - n, big, dtype=np.int64)])
    span = big + 1
    s, w = 0, 1
    while w < size:
        blocks = a.reshape(-1, 2, w)
        rows = np.arange(len(blocks), dtype=np.int64)[:, None] * span
        left = (blocks[:, 0, :] + rows).ravel()
        right = blocks[:, 1, :] + rows
        lb = np.searchsorted(left, right, "left") - rows // span * w
        ub = np.searchsorted(left, right, "right") - rows // span * w
        s += int((lb - (w - ub)).sum())
        a = np.sort(blocks.reshape(-1, 2 * w), axis=1).ravel()
        w *= 2
    return s - n * (size - n)


def _mk(eng, runs):
    values = np.concatenate([np.asarray(r, dtype=np.uint32) for r in runs]) if runs else np.zeros(0, np.uint32)
    first = np.concatenate([[0], np.cumsum([len(r) for r in runs])]).astype(np.uint64)
    s, t = eng.mk_stats(values, first)
    return s.tolist(), [int(v) for v in t.tolist()]


def test_merge_count_oracle_itself():
    rng = np.random.default_rng(3)
    for n in (0, 1, 2, 5, 100, 777, 4097):
        for hi in (3, 1000, 2 ** 32):
            x = rng.integers(0, hi, size=n)
            assert _merge_count(x) == _sign_matrix(x)[0], (n, hi)


LENGTHS = [0, 1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]


KINDS = ["wide", "narrow", "equal", "sorted", "reversed"]


@pytest.mark.parametrize("kind", KINDS)
def test_mk_stats_against_sign_matrix(kind):
    """runs of every length around the wave / tile / level boundaries and random lengths in one call; values all distinct,
    heavily tied, all equal, sorted, reversed"""
    from ntjoin_amd.engine import MxEngine
    rng = np.random.default_rng(100 + KINDS.index(kind))
    lengths = LENGTHS + rng.integers(2, 5000, size=24).tolist() + [4 * T + 3, 30_000 if kind == "wide" else 9000]
    rng.shuffle(lengths)
    runs = []
    for n in lengths:
        if kind == "wide":
            x = rng.permutation(np.unique(rng.integers(0, 2 ** 32, size=n + 64)))[:n]
        elif kind == "narrow":
            x = rng.integers(0, 7, size=n)
        elif kind == "equal":
            x = np.full(n, 12345)
        elif kind == "sorted":
            x = np.sort(rng.integers(0, 2 ** 32, size=n))
        else:
            x = np.sort(rng.integers(0, 2 ** 32, size=n))[::-1]
        runs.append(np.asarray(x, dtype=np.uint32))
    with MxEngine(k=32, w=10) as eng:
        s, t = _mk(eng, runs)
    for i, x in enumerate(runs):
        assert (s[i], t[i]) == _sign_matrix(x), (kind, len(x))


def test_mk_stats_long_runs_closed_forms():
    """B increasing blocks of b in reverse block order: s = B b(b-1)/2 - B(B-1)/2 b^2 (n = 4 194 000, not a multiple of the
    tile); a reversed run of 2^22: s = -n(n-1)/2; a random permutation of 10^6 + 17 against the numpy merge count; and a group
    of 2 * 10^6 equal values, whose tie term is just below 2^64"""
    from ntjoin_amd.engine import MxEngine
    B, b = 4194, 1000
    blocks = np.concatenate([np.arange(k * b, (k + 1) * b) for k in range(B - 1, -1, -1)])
    n2 = 1 << 22
    rev = np.arange(n2)[::-1]
    perm = np.random.default_rng(8).permutation(1_000_017)
    t_eq = 2_000_000
    runs = [blocks, np.arange(5), rev, perm, np.full(t_eq, 7), np.array([4, 4, 1])]
    with MxEngine(k=32, w=10) as eng:
        s, t = _mk(eng, runs)
    assert s[0] == B * b * (b - 1) // 2 - B * (B - 1) // 2 * b * b and t[0] == 0
    assert (s[1], t[1]) == (10, 0)
    assert s[2] == -n2 * (n2 - 1) // 2 and t[2] == 0
    assert s[3] == _merge_count(perm) and t[3] == 0
    assert s[4] == 0 and t[4] == t_eq * (t_eq - 1) * (2 * t_eq + 5) < 2 ** 64
    assert (s[5], t[5]) == (-2, 18)


def test_mk_stats_errors():
    from ntjoin_amd import capi
    from ntjoin_amd.engine import MxEngine, MxError
    with MxEngine(k=32, w=10) as eng:
        with pytest.raises(MxError) as ei:  # 3 * 10^6 equal values: t(t-1)(2t+5) > 2^64 - 1
            eng.mk_stats(np.zeros(3_000_000, dtype=np.uint32), [0, 3_000_000])
        assert ei.value.code == capi.MXG_ELIMIT
        with pytest.raises(MxError):
            eng.mk_stats(np.zeros(10, dtype=np.uint32), [0, 6, 4, 10])
        s, t = eng.mk_stats(np.zeros(0, dtype=np.uint32), [0])
        assert len(s) == len(t) == 0
        assert eng.mk_stats(np.array([5, 1, 9], dtype=np.uint32), [0, 3])[0].tolist() == [1]  # the handle still works


def test_path_segments_mk_needs_path_segments_of_that_assembly():
    from ntjoin_amd.engine import MxEngine, MxError
    rng = np.random.default_rng(2)
    hs = np.unique(rng.integers(1, 2 ** 63, size=300, dtype=np.uint64))[:200]
    pos = (np.arange(200, dtype=np.uint32) * 7)
    with MxEngine(k=32, w=10) as eng:
        eng.add_minimizers("a", 2.0, hs, pos, np.zeros(200, np.uint32), ["c"])
        eng.add_minimizers("b", 1.0, hs[::-1].copy(), pos, np.zeros(200, np.uint32), ["d"])
        eng.build_graph()
        eng.find_paths(1)
        with pytest.raises(MxError):
            eng.path_segments_mk(1)
        eng.path_segments(0)
        with pytest.raises(MxError):
            eng.path_segments_mk(1)
        assert eng.path_segments_mk(0)["s"].tolist() == [200 * 199 // 2]
        eng.path_segments(1)
        assert eng.path_segments_mk(1)["s"].tolist() == [-200 * 199 // 2]
        eng.find_paths(1)  # new paths: the segments before them are gone
        with pytest.raises(MxError):
            eng.path_segments_mk(1)


# ---- the path route on assemblies made to need the test ----------------------------------------------------------------
def _swap_pairs(codes, b=200):
    n = len(codes) // (2 * b) * (2 * b)
    return codes[:n].reshape(-1, 2, b)[:, ::-1, :].reshape(-1).copy()


def _rc(codes):
    return (np.uint8(3) - codes)[::-1].copy()


def _write_fasta(path, records):
    from ntjoin_amd import synth
    with open(path, "w", encoding="ascii") as fh:
        for rid, codes in records:
            fh.write(f">{rid}\n{synth.to_ascii(codes).decode()}\n")


def _host_orientation(ps):
    from ntjoin_amd.ntjoin import mk_orientation
    if len(ps) > 1:
        d = np.diff(np.asarray(ps, dtype=np.int64))
        if (d > 0).all():
            return "+"
        if (d < 0).all():
            return "-"
        return mk_orientation(len(ps), _merge_count(ps), _tie_term(ps))
    return "?"


def test_path_route_and_format_paths_mkt(tmp_path):
    """a reference of 8 Mbp and a target cut from it (w = 100, weights 2 / 1, -n 2): a plain contig, contigs with every adjacent
    pair of 200 bp blocks swapped (about 7 of 8 consecutive pairs increasing: the m rule leaves them out, Mann-Kendall orients
    them), one of them reverse-complemented, one block-shuffled, and one of 6 Mbp whose run has more than 50 000 vertices"""
    from ntjoin_amd import synth
    from ntjoin_amd.ntjoin import Ntjoin
    ref = synth.make_reference(21, 8_000_000)[0]
    rng = np.random.default_rng(22)
    shuf = ref[1_100_000:1_300_000].reshape(-1, 200)
    tgt = [("plain", ref[50_000:350_000]), ("swap", _swap_pairs(ref[400_000:700_000])),
           ("swap_rc", _rc(_swap_pairs(ref[750_000:1_050_000]))),
           ("shuffled", shuf[rng.permutation(len(shuf))].reshape(-1)), ("long", _swap_pairs(ref[1_400_000:7_400_000]))]
    os.chdir(tmp_path)
    _write_fasta("ref.fa", [("chr", ref)])
    _write_fasta("tgt.fa", tgt)
    names = {"ref.fa.k32.w100.tsv": "ref.fa", "tgt.fa.k32.w100.tsv": "tgt.fa"}
    args = argparse.Namespace(FILES=["ref.fa.k32.w100.tsv"], s="tgt.fa.k32.w100.tsv", l=1, p=str(tmp_path / "out"), k=32, n=2,
                              t=1)
    nj = Ntjoin(args, fasta={k: str(tmp_path / v) for k, v in names.items()}, w=100)
    try:
        nj.weights_list = [2]
        with contextlib.redirect_stdout(io.StringIO()):
            nj.load_minimizers_scaffold()
            nj.make_minimizer_graph(materialize=False)
            found = nj.find_paths()
        got_mkt = nj.format_paths(mkt=True)
        got_m = nj.format_paths(mkt=False)
        eng, tgt_a = nj._engine, 1
        seg = eng.path_segments(tgt_a)
        mk = eng.path_segments_mk(tgt_a)
        gr = eng.get_graph()
        vpos, vrec = gr["vertex_pos"][tgt_a], gr["vertex_record"][tgt_a]
        ids = eng.record_ids(tgt_a, eng.n_records(tgt_a))
        paths = nj._found
    finally:
        nj.close()
    assert sum(len(c) for c in found) >= 1
    # (1) the statistics of every run against the host, from the path vertices and the graph's positions
    verts = np.concatenate([np.asarray(v, dtype=np.int64) for _c, v in paths])
    ends = np.append(seg["first"].astype(np.int64)[1:], len(verts))
    longest = 0
    for i, (f, e) in enumerate(zip(seg["first"].tolist(), ends.tolist())):
        ps = vpos[verts[f:e]].astype(np.int64)
        assert len(ps) == int(seg["n"][i])
        assert (int(mk["s"][i]), int(mk["tie_term"][i])) == (_merge_count(ps), 0), (i, ids[int(seg["record"][i])], len(ps))
        longest = max(longest, len(ps))
    assert longest > 50_000
    # (2) format_paths(mkt=True) against format_path restated on the host with the Mann-Kendall decision
    for p, (_c, pverts) in enumerate(paths):
        runs = []
        for v in pverts:
            ctg = ids[int(vrec[v])]
            if runs and runs[-1][0] == ctg:
                runs[-1][1].append(int(vpos[v]))
            else:
                runs.append((ctg, [int(vpos[v])]))
        want = [(ctg, ori) for ctg, ori in ((c, _host_orientation(ps)) for c, ps in runs) if ori != "?"]
        assert [(node[0], node[1]) for node in got_mkt[p]] == want, p
    # (3) the test's teeth: runs the m rule leaves out and Mann-Kendall orients
    oriented_mkt = {(p, node[0]) for p, nodes in enumerate(got_mkt) for node in nodes}
    oriented_m = {(p, node[0]) for p, nodes in enumerate(got_m) for node in nodes}
    assert oriented_m < oriented_mkt
    assert {c for _p, c in oriented_mkt - oriented_m} >= {"swap", "swap_rc", "long"}


def _fasta_lengths(path):
    lens, rid = {}, None
    for line in open(path, encoding="ascii"):
        if line.startswith(">"):
            rid = line[1:].split()[0]
            lens[rid] = 0
        elif rid is not None:
            lens[rid] += len(line.strip())
    return lens


@pytest.mark.parametrize("name", [m["name"] for m in golden_cases()])
def test_format_paths_mkt_on_goldens(name):
    """every run of the 20 golden cases at every -n is strictly monotone, so --mkt changes nothing: format_paths(mkt=True)
    equals the reference's own format_path output"""
    from ntjoin_amd.ntjoin import Ntjoin
    case = load_case(name)
    meta, ref = case["meta"], case["reference"]
    fa = ref["format_args"]
    lengths = _fasta_lengths(os.path.join(GOLDEN, "fasta", meta["target"]["fasta"]))
    cwd = os.getcwd()
    os.chdir(os.path.join(GOLDEN, "cases", name))
    try:
        for n, want in ref["format_by_n"].items():
            args = argparse.Namespace(FILES=[r["tsv"] for r in meta["refs"]], s=meta["target"]["tsv"],
                                      l=meta["target"]["weight"], p="/tmp/mxg_mkt_" + name, k=meta["k"], n=int(n), t=1)
            nj = Ntjoin(args, variant=meta["variant"])
            try:
                nj.weights_list = [r["weight"] for r in meta["refs"]]
                with contextlib.redirect_stdout(io.StringIO()):
                    nj.load_minimizers_scaffold()
                    nj.make_minimizer_graph(materialize=False)
                    nj.find_paths()
                got = nj.format_paths(lengths, g=fa["g"], G=fa["G"], m=fa["m"], mkt=True)
            finally:
                nj.close()
            key = lambda nodes: tuple(tuple(x) for x in nodes)  # noqa: E731
            assert sorted(map(key, got)) == sorted(map(key, want)), (name, n)
    finally:
        os.chdir(cwd)
