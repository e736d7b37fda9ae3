"""CPU tests of the --mkt orientation decision (reference bin/ntjoin_assemble.py:37-40: pymannkendall.original_test on every
run that is not strictly monotone): ntjoin_amd.ntjoin.mk_orientation on known answers, against scipy and pymannkendall where
they are installed, and the mkt switch of Ntjoin.format_paths on a stand-in engine."""
import argparse
import math
import random
import types

import numpy as np
import pytest

from ntjoin_amd.ntjoin import MK_Z975, Ntjoin, mk_orientation


def _s_ties(x):
    """pairwise restatement: s = sum over i < j of sign(x_j - x_i), tie term = sum over groups of t(t-1)(2t+5)"""
    n = len(x)
    s = sum((x[j] > x[i]) - (x[j] < x[i]) for i in range(n) for j in range(i + 1, n))
    counts = {}
    for v in x:
        counts[v] = counts.get(v, 0) + 1
    return s, sum(t * (t - 1) * (2 * t + 5) for t in counts.values())


FIRST = [0, 1, 2, 3, 5, 4, 6, 7, 8, 9]
KNOWN = [  # values, s, var, z, decision (pairwise counts and scipy on the build machine)
    (FIRST, 43, 125.0, 3.7566, "+"),
    ([1, 2, 3, 5, 4], 8, 16.667, 1.7146, "?"),
    ([3, 1, 4, 1, 5, 9, 2, 6, 5, 3], 12, 122.0, 0.9959, "?"),
    (FIRST[::-1], -43, 125.0, -3.7566, "-"),
]


@pytest.mark.parametrize("x,s,var,z,want", KNOWN)
def test_known_answers(x, s, var, z, want):
    n = len(x)
    got_s, tie = _s_ties(x)
    assert got_s == s
    v = (n * (n - 1) * (2 * n + 5) - tie) / 18
    assert v == pytest.approx(var, abs=1e-3)
    assert (got_s - 1 if got_s > 0 else got_s + 1) / math.sqrt(v) == pytest.approx(z, abs=5e-5)
    assert mk_orientation(n, s, tie) == want


def test_known_tie_term():
    assert _s_ties([3, 1, 4, 1, 5, 9, 2, 6, 5, 3])[1] == 54
    assert mk_orientation(1, 0, 0) == "?" and mk_orientation(5, 0, 5 * 4 * 15) == "?"   # one value; all equal


def test_mkt_decides_where_the_m_rule_does_not():
    """8 of 9 consecutive pairs increasing: 88.9 % < m = 90 gives '?', the Mann-Kendall test '+'"""
    n, inc, dec = 10, 8, 1
    assert Ntjoin.determine_orientation(n, inc, dec, 90) == "?"
    assert Ntjoin._orientation_mkt(n, inc, dec, 43, 0) == "+"
    assert Ntjoin._orientation_mkt(n, 0, 9, 0, 0) == "-"        # strictly monotone: decided before the test
    assert Ntjoin._orientation_mkt(1, 0, 0, 0, 0) == "?"


def test_threshold_is_scipy_ppf():
    stats = pytest.importorskip("scipy.stats")
    assert MK_Z975 == stats.norm.ppf(0.975)


def test_decision_equals_scipy_for_every_reachable_s():
    """every (n, s) a run of n distinct values can have, n <= 200: scipy's h and p <= 0.05 (original_test's formulas)"""
    stats = pytest.importorskip("scipy.stats")
    ppf = stats.norm.ppf(0.975)
    for n in range(2, 201):
        smax = n * (n - 1) // 2
        s = np.arange(-smax, smax + 1, 2, dtype=np.int64)     # s = smax - 2 * (inversions)
        var = (n * (n - 1) * (2 * n + 5)) / 18
        z = np.where(s > 0, (s - 1) / np.sqrt(var), np.where(s < 0, (s + 1) / np.sqrt(var), 0.0))
        p = 2 * (1 - stats.norm.cdf(np.abs(z)))
        h = np.abs(z) > ppf
        want = np.where(h & (p <= 0.05), np.where(z > 0, "+", "-"), "?")
        got = [mk_orientation(n, int(v), 0) for v in s.tolist()]
        assert got == want.tolist(), n


def test_s_is_kendall_tau_numerator():
    """s = the numerator of tau_b(range(n), x) (= concordant - discordant pairs), with and without ties"""
    stats = pytest.importorskip("scipy.stats")
    rng = random.Random(11)
    for trial in range(60):
        n = rng.randint(2, 120)
        hi = rng.choice([3, 10, 10 ** 6])
        x = [rng.randrange(hi) for _ in range(n)]
        s, _ = _s_ties(x)
        n0 = n * (n - 1) // 2
        n1 = sum(t * (t - 1) // 2 for t in (x.count(v) for v in set(x)))
        if n1 == n0:
            assert s == 0
            continue
        tau = stats.kendalltau(range(n), x).statistic
        assert round(tau * math.sqrt(n0 * (n0 - n1))) == s, (trial, x)


def test_decision_equals_pymannkendall():
    mk = pytest.importorskip("pymannkendall")
    rng = random.Random(5)
    for trial in range(400):
        n = rng.randint(3, 150)
        hi = rng.choice([4, 30, 10 ** 6])
        drift = rng.choice([-0.02, 0.0, 0.01, 0.05])
        x = [rng.randrange(hi) + int(drift * i * hi) for i in range(n)]
        r = mk.original_test(x)
        want = ("+" if r.trend == "increasing" else "-") if (r.h and r.p <= 0.05) else "?"
        s, tie = _s_ties(x)
        assert mk_orientation(n, s, tie) == want, (trial, x)


class _StubEngine:
    """what format_paths asks of MxEngine for one path that is one run of the target's contig ctg0"""

    def __init__(self, pos):
        self.pos = pos

    def record_ids(self, a, n):
        return ["ctg0"]

    def n_records(self, a):
        return 1

    def record_lengths(self, a):
        return [100_000]

    def mx_extremes(self, a):
        return [(min(self.pos), max(self.pos))]

    def path_segments(self, a):
        pairs = list(zip(self.pos, self.pos[1:]))
        col = lambda v: np.array([v], dtype=np.uint32)  # noqa: E731
        return {"path": col(0), "record": col(0), "first": col(0), "n": col(len(self.pos)), "min_pos": col(min(self.pos)),
                "max_pos": col(max(self.pos)), "inc": col(sum(a < b for a, b in pairs)), "dec": col(sum(a > b for a, b in pairs))}

    def path_segments_mk(self, a):
        s, tie = _s_ties(self.pos)
        return {"s": np.array([s], dtype=np.int64), "tie_term": np.array([tie], dtype=np.uint64)}

    def get_graph(self):
        e = np.arange(len(self.pos) - 1, dtype=np.uint32)
        return {"vertex_pos": np.array([self.pos], dtype=np.uint32), "edge_u": e, "edge_v": e + 1,
                "edge_support": np.ones(len(e), dtype=np.uint32)}


def _stub_ntjoin(pos):
    nj = Ntjoin.__new__(Ntjoin)
    nj.args = argparse.Namespace(k=32)
    nj._engine = _StubEngine(pos)
    nj._order = ["tgt"]
    nj._found = [(0, list(range(len(pos))))]
    nj._graph, nj._graph_pending = types.SimpleNamespace(names=[f"v{i}" for i in range(len(pos))]), False
    return nj


def test_format_paths_mkt_switch():
    """format_paths(mkt=True) orients the run the m rule leaves out; mkt=False is the m rule"""
    nj = _stub_ntjoin([100 * v for v in FIRST])
    assert nj.format_paths() == [[]]
    assert nj.format_paths(mkt=False) == [[]]
    assert nj.format_paths(mkt=True) == [[["ctg0", "+", 0, 100_000, 100_000, "v0", "v9", 0, 0]]]
    nj = _stub_ntjoin([100 * v for v in [1, 2, 3, 5, 4]])
    assert nj.format_paths(mkt=True) == [[]] and nj.format_paths(m=75) != [[]]
