"""CPU tests of the path stage's boundary (mxg_format_paths / mxg_mk_orientation): the Mann-Kendall decision the library takes
on the host against ntjoin_amd.ntjoin.mk_orientation, the two structs of the call against the sizes the library asserts, and the
host route of Ntjoin.format_paths for an engine without the call.  The library loads without a GPU, as test_capi_cpu relies on."""
import ctypes as C
import os

from ntjoin_amd.ntjoin import Ntjoin, mk_orientation
from tests.conftest import REPO
from tests.test_mkt_cpu import FIRST, _s_ties, _stub_ntjoin

FORMAT_PARAMS_BYTES = 40      # u32 + pad, i64, i64, f64, u32 + pad   (static_assert in csrc/api.cpp)
PATH_NODES_VIEW_BYTES = 104   # 2 x u64 + 11 pointers                 (static_assert in csrc/api.cpp)


def _lib():
    from ntjoin_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi, capi.load()


def _decide(lib, n, s, tie):
    return lib.mxg_mk_orientation(n, s, tie).decode()


def test_mk_orientation_equals_python_for_every_reachable_s():
    """every 2 <= n <= 60 and every s of the right parity in [-n(n-1)/2, n(n-1)/2] without ties: the sweep crosses |z| = 1.96
    for every n >= 5, where another erfc would show"""
    _, lib = _lib()
    crossed = set()
    for n in range(2, 61):
        smax = n * (n - 1) // 2
        seen = set()
        for s in range(-smax, smax + 1, 2):
            want = mk_orientation(n, s, 0)
            assert _decide(lib, n, s, 0) == want, (n, s)
            seen.add(want)
        if seen == {"+", "-", "?"}:
            crossed.add(n)
    assert crossed == set(range(5, 61))


def test_mk_orientation_equals_python_with_ties():
    """tied samples: one group of 2, of 3 and of n / 2 equal values, every s the rest can still give (and beyond: the decision
    is a function of the three integers)"""
    _, lib = _lib()
    for n in range(4, 61):
        for t in (2, 3, n // 2):
            tie = t * (t - 1) * (2 * t + 5)
            smax = n * (n - 1) // 2 - t * (t - 1) // 2
            for s in range(-smax, smax + 1):
                assert _decide(lib, n, s, tie) == mk_orientation(n, s, tie), (n, t, s)
    assert _decide(lib, 1, 0, 0) == "?" and _decide(lib, 5, 0, 5 * 4 * 15) == "?"   # one value; all equal


def test_mk_orientation_on_the_runs_of_test_mkt_cpu():
    _, lib = _lib()
    for x, want in ((FIRST, "+"), ([1, 2, 3, 5, 4], "?"), (FIRST[::-1], "-"), ([3, 1, 4, 1, 5, 9, 2, 6, 5, 3], "?")):
        s, tie = _s_ties(x)
        assert _decide(lib, len(x), s, tie) == mk_orientation(len(x), s, tie) == want


def test_mk_orientation_long_runs_round_like_python():
    """n(n-1)(2n+5) beyond 2^53: the variance is the exact integer divided by 18 and rounded once, as int / int is in Python"""
    _, lib = _lib()
    for n in (165_000, 208_064, 1_000_003, 50_000_017, 2 ** 31 - 1):
        var = n * (n - 1) * (2 * n + 5) / 18
        z196 = int(1.959963984540054 * var ** 0.5)
        for tie in (0, 6 * 5 * 17, 1000 * 999 * 2005):
            for s in range(z196 - 40, z196 + 40):
                assert _decide(lib, n, s, tie) == mk_orientation(n, s, tie), (n, s, tie)
                assert _decide(lib, n, -s, tie) == mk_orientation(n, -s, tie), (n, -s, tie)


def test_symbols_bound_and_struct_sizes():
    capi, lib = _lib()
    for name in ("mxg_format_paths", "mxg_mk_orientation", "mxg_vertex_hashes"):
        assert name in capi.SYMBOLS and hasattr(lib, name)
    assert C.sizeof(capi.FormatParams) == FORMAT_PARAMS_BYTES
    assert C.sizeof(capi.PathNodesView) == PATH_NODES_VIEW_BYTES
    api = open(os.path.join(REPO, "ntjoin_amd", "csrc", "api.cpp"), encoding="utf-8").read()
    assert f"static_assert(sizeof(mxg_format_params) == {FORMAT_PARAMS_BYTES}," in api
    assert f"static_assert(sizeof(mxg_path_nodes_view) == {PATH_NODES_VIEW_BYTES}," in api
    assert [f for f, _ in capi.FormatParams._fields_] == ["struct_size", "g", "G", "m", "mkt"]
    assert [f for f, _ in capi.PathNodesView._fields_] == [
        "n_paths", "n_nodes", "node_first", "record", "start", "end", "contig_size", "reverse", "first_vertex",
        "terminal_vertex", "gap_size", "raw_gap_size", "segment"]


def test_engine_without_the_call_goes_the_host_route():
    """the stand-in engine of test_mkt_cpu has no format_paths: Ntjoin.format_paths is _format_paths_host there"""
    pos = [100 * v for v in FIRST]
    nj = _stub_ntjoin(pos)
    assert not hasattr(nj._engine, "format_paths")
    want = [[["ctg0", "+", 0, 100_000, 100_000, "v0", "v9", 0, 0]]]
    assert nj.format_paths(mkt=True) == nj._format_paths_host(mkt=True) == want
    assert nj.format_paths(m=75) == nj._format_paths_host(m=75) == want
    assert nj.format_paths() == nj._format_paths_host() == [[]]
    calls = []
    nj._format_paths_host = lambda *a: calls.append(a) or "host"
    assert nj.format_paths({"ctg0": 5}, 1, 2, 3, True) == "host" and calls == [({"ctg0": 5}, 1, 2, 3, True)]
    assert callable(Ntjoin._format_paths_host)
